"""The ledger of tests/test_gpu_framed_buffers.py, held against the exports without a device: every export that takes a
c_void_p has a framed case there or a written-out reason not to, so a new export without a case fails here.  And the helper's
pattern, `check` and `unwritten` on CPU tensors."""
import ctypes as C

import pytest
import torch

import framed_util as fu
import test_gpu_framed_buffers as G
from ecg_denoise_amd import _lib


def _with_pointer():
    return {name for name, (_, args) in _lib._SIGS.items() if C.c_void_p in args}


def test_every_export_with_a_pointer_has_a_case_or_a_reason():
    assert set(_lib.EXPORTS) == set(_lib._SIGS)
    need = _with_pointer() - set(G.LEDGER_EXEMPT)
    have = set(G.CASES)
    assert have == need, f"without a framed case: {sorted(need - have)}; claimed but no such export: {sorted(have - need)}"
    assert set(G.LEDGER_EXEMPT) <= set(_lib.EXPORTS), sorted(set(G.LEDGER_EXEMPT) - set(_lib.EXPORTS))
    assert all(isinstance(r, str) and len(r) > 10 for r in G.LEDGER_EXEMPT.values())
    # what the issue allows to be left out, and nothing else
    allowed = {"ral_create", "ral_destroy", "ral_bind", "ral_set_option", "ral_debug_tensor", "ral_mix_draw", "ral_pe_table"}
    assert all(n in allowed or n.startswith(("ral_grad_bucket", "ral_profile_")) for n in G.LEDGER_EXEMPT), sorted(G.LEDGER_EXEMPT)


def test_every_claim_names_a_test_of_the_gpu_file():
    for entry, tests in G.CASES.items():
        assert tests, entry
        for t in tests:
            fn = getattr(G, t, None)
            assert callable(fn) and t.startswith("test_") and entry in fn._entries, (entry, t)


def test_every_exemption_names_a_pointer_argument_and_gives_a_reason():
    for (name, i), why in G.EXEMPT.items():
        args = _lib._SIGS[name][1]
        assert 0 <= i < len(args) and args[i] is C.c_void_p, (name, i)
        assert isinstance(why, str) and why, (name, i)
    # a device buffer is never exempt: the exemptions are handles, streams, host tables and host out-parameters
    assert {w.split(" ")[0] for w in G.EXEMPT.values()} == {"the", "host"}
    handles = {k for k, w in G.EXEMPT.items() if w == "the handle"}
    assert all(i == 0 for _, i in handles)
    streams = {k for k, w in G.EXEMPT.items() if w == "the stream"}
    assert all(i == len(_lib._SIGS[n][1]) - 1 for n, i in streams)


def test_pattern_check_and_unwritten_on_cpu_tensors():
    reg = fu.Registry()
    a = reg.framed((3, 5), torch.float32, "cpu")
    assert a.data_ptr() % fu.ALIGN == 0 and tuple(a.shape) == (3, 5)
    assert torch.isnan(a).all() and (a.view(torch.int32) == fu.WORD).all() and fu.unwritten(a) == 15
    e = reg.entry_of(a)
    assert e.off >= fu.FRAME and e.nbytes == 60 and e.raw.numel() >= 2 * fu.FRAME + 60
    assert (e.raw[e.off - fu.FRAME:e.off].view(torch.int32) == fu.WORD).all()
    a[0, 0], a[1, 1] = 1.0, float("nan")
    assert fu.unwritten(a) == 13 and fu.unwritten(a[1]) == 4            # a NaN result is not the pattern
    reg.check_all()
    d = reg.framed(7, torch.float64, "cpu")                             # finite as fp64: only the bits tell
    assert torch.isfinite(d).all() and fu.unwritten(d) == 7
    d[3] = 0.0
    assert fu.unwritten(d) == 6
    i = reg.framed((4,), torch.int64, "cpu", fill=torch.arange(4))
    f = reg.framed((2, 2), torch.float32, "cpu", fill=0.5)
    assert i.tolist() == [0, 1, 2, 3] and (f == 0.5).all() and fu.unwritten(i) == 0 and fu.unwritten(f) == 0
    z = reg.framed((0,), torch.float64, "cpu")                          # zero length: the two frames touch
    ez = reg.entry_of(z)
    assert z.numel() == 0 and ez.nbytes == 0 and reg.find(ez.ptr) is ez and fu.unwritten(z) == 0
    reg.check_all()


def test_check_names_the_buffer_the_side_and_the_offset():
    reg = fu.Registry()
    a = reg.framed((3, 5), torch.float32, "cpu", name="out")
    e = reg.entry_of(a)
    e.raw[e.off + e.nbytes:e.off + e.nbytes + 4].view(torch.float32).fill_(2.0)      # one element past the end
    with pytest.raises(fu.FrameError, match=r"out: rear frame damaged, first damaged byte 0 byte\(s\) past the end"):
        reg.check(a)
    e.raw[e.off + e.nbytes:e.off + e.nbytes + 4].view(torch.int32).fill_(fu.WORD)
    reg.check(a)
    e.raw[e.off + e.nbytes + 4 * 7 + 1] = 0                                         # a byte of the 8th word behind the payload
    with pytest.raises(fu.FrameError, match=r"rear frame damaged, first damaged byte 29 "):
        reg.check_all()
    e.raw[e.off + e.nbytes + 4 * 7 + 1] = 0xA5
    e.raw[e.off - 4:e.off].view(torch.float32).fill_(0.0)                            # element [-1]
    with pytest.raises(fu.FrameError, match=r"out: front frame damaged, first damaged byte 1 byte\(s\) before the start of the payload, the damage reaches byte 4 "):
        reg.check(a)


def test_proxy_refuses_a_pointer_outside_every_payload():
    reg = fu.Registry()
    x = reg.framed((8,), torch.float32, "cpu", fill=0.0)
    plain = torch.zeros(8)
    calls = []

    class Lib:
        def ral_wavelet_denoise(self, *a):
            calls.append(a)
            return 0

        def ral_last_error(self):
            return b""

    proxy = fu.AbiProxy(Lib(), _lib._SIGS, reg, {("ral_wavelet_denoise", 5): "the stream"})
    p = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
    assert proxy.ral_wavelet_denoise(p(x), p(x, 16), 1, 4, 0.04, C.c_void_p(12345)) == 0        # an offset into a payload is fine
    assert proxy.ral_wavelet_denoise(p(x), None, 1, 4, 0.04, 12345) == 0                          # so is a null pointer
    with pytest.raises(fu.FrameError, match=r"ral_wavelet_denoise: argument 1 "):
        proxy.ral_wavelet_denoise(p(x), p(plain), 1, 4, 0.04, C.c_void_p(12345))
    with pytest.raises(fu.FrameError, match=r"ral_wavelet_denoise: argument 0 "):
        proxy.ral_wavelet_denoise(x.data_ptr() - 4, p(x), 1, 4, 0.04, C.c_void_p(12345))          # the front frame is not the payload
    assert len(calls) == 2 and proxy.seen == {"ral_wavelet_denoise"} and proxy.ral_last_error() == b""


def test_framed_factories_leave_cpu_allocations_alone_and_restore_torch():
    reg = fu.Registry()
    before = (torch.empty, torch.zeros, torch.full, torch.ones, torch.empty_like, torch.zeros_like, torch.full_like, torch.cat)
    with fu.framed_factories(reg, concat=True):
        assert torch.empty is not before[0]
        t = torch.zeros(3, 2)
        u = torch.full((2,), 3, dtype=torch.int64)
        v = torch.cat([t, t])
    assert (torch.empty, torch.zeros, torch.full, torch.ones, torch.empty_like, torch.zeros_like, torch.full_like, torch.cat) == before
    assert not reg.entries and tuple(t.shape) == (3, 2) and u.tolist() == [3, 3] and tuple(v.shape) == (6, 2)
    with pytest.raises(ZeroDivisionError):
        with fu.framed_factories(reg):
            1 / 0
    assert torch.empty is before[0]
