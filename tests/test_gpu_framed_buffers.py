"""No entry point writes or reads outside its caller's buffers: every case runs on framed buffers (tests/framed_util.py).

Every case frames everything that crosses the C ABI - an `AbiProxy` in front of the loaded library refuses any device pointer
that lies in no framed payload - fills scratch, outputs and the regions the header calls never-read with the pattern
0x7FC0A5A5, runs, synchronises, checks every frame bit for bit, checks that the outputs the header says are written hold no
pattern word, and compares the results with the same call on ordinary tensors: bit for bit where the suite asserts run-to-run
bit equality (eval forwards, the streaming and analysis kernels, fft / wavelet, mix_records / score_records / mix_batch), at the
bar of the quantity's own oracle test where floating-point atomics are involved (1e-4 relative L2 for parameter gradients and
what follows from training-mode BatchNorm sums, tests/test_gpu_parity.py; 2e-5 for the attention operator,
tests/test_gpu_attention.py; 1e-5 for a training forward, the bar of smoke()).

Covered entry points and their framed buffers (CASES below is the machine-readable form; tests/test_framed_ledger_cpu.py holds
it against `_lib.EXPORTS`):

  model handles (test_model_handle, test_newrale_handle, test_split_ralenet, test_split_unet)
    ral_forward, ral_forward_loss_means, ral_loss, ral_backward, ral_adam_step     params, grads, adam_m, adam_v, state, bn_sums
    ral_forward_begin / _end, ral_backward_begin / _end, ral_backward_input,       at exactly ral_param_floats / ral_state_floats /
    ral_backward_input_begin / _end, ral_unet_forward_stage / _finish,             ral_bn_sums_doubles elements (zero-length bn_sums
    ral_unet_backward_start / _stage / _finish                                     for ACDAE and DANet); x, target, y, dy, dx, snr,
                                                                                   rmse, means3, scratch64, loss_sum
    ral_conv13_forward / _backward, ral_adam_flat, ral_loss_means (NewRALE)        the adapter's flat params / grads / adam_m / adam_v
  stateless operators, raw ABI, scratch at exactly the queried size
    ral_attention_forward / _backward   qkv, o, lse, table, d_o, gtable, dqkv, scratch (ral_attention_backward_scratch_floats)
    ral_loss_flat / _mean / _means      pred, target, dy, snr, rmse, loss_sum[1], loss_mean[1], scratch2[2], means3[3], scratch64[64]
    ral_adam_flat                       p, g, m, v
    ral_conv13_forward / _backward      x, w, b, y, dy, gw, gb, dx
    ral_wavelet_denoise                 x, y
    ral_fft_denoise                     x, y, kept, scratch (ral_fft_denoise_scratch_bytes)
    ral_prep_windows                    sig, noise, sums[2 leads + 1], noisy, clean
    ral_stream_windows / _stitch        rec, win, stats, y, out
    ral_mix_records, ral_score_records  rec, noise, scratch (queried bytes, rounded up to 8), noisy, clean; the four score tables
    ral_beat_records                    x, bank, scratch (queried bytes, rounded up to 8), peaks, count
  through the wrappers, framed allocation active
    ral_live_windows / _emit, ral_pool_windows / _emit                     hist (pattern-filled: a new stream), x, win, stats, y, out,
    ral_newrale_stream_front / _back, ral_newrale_live_front / _back,      last_y, last_stats, table_dev, adapter_params
    ral_newrale_pool_front / _back, ral_stream_windows / _stitch
    ral_mix_batch                                                          bank, noise, rows, noisy, clean, draws, snr_db
    ral_rate_records, ral_rate_pool                                        x, bank, y, hist (pattern-filled), table_dev, out
    ral_beat_records, ral_beat_pool, ral_beat_match                        x, bank, scratch, peaks, count, hist (pattern-filled)
    ral_rhythm_records, ral_rhythm_pool                                    x, peaks, count, label, corr, rr_ratio, ring, ring_pos,
                                                                           new_pos, scratch (exactly the queried bytes), out_pos
    ral_delineate_records, ral_pst_records, ral_template_records,          x, peaks (cap = the largest count), count, labels, on, off and
    ral_hrv_windows, ral_arrhythmia_windows                                every output; band; table_dev

Shapes that an entry point's own rules refuse: the U-Net provides no input gradient and refuses a non-NULL dx, so its cases run
ral_backward without dx; DANet's wrapper counts its shared BatchNorms in a forward of its own, so its forward_loss is ral_forward +
ral_loss_means instead of ral_forward_loss_means.  Every other named shape ran as named.

Observed run time of the file on an MI355X: 65 cases in 11 s (the two attention subprocesses 4 s each, the 8 M-float optimiser
case 0.5 s, every other case well under a second).

Findings (each case above passes; no frame was ever damaged and no output kept a pattern word):
  1. ral_backward of a U-Net that sums its weight gradients from per-workgroup rows (the "fold", (2, 256) here) wrote every
     parameter's gradient but never the padding floats between the tensors of the flat layout (6 floats at (2, 256): offsets 5026,
     5027, 5030, 5031, 5034, 5035), although the header says `grads` is zeroed first; ral_adam_step runs over the whole buffer and
     turned what lay there into params / adam_m / adam_v (with the fix reverted test_model_handle[unet-2x256-*] fails with
     "grads: 6 floats between the parameters keep what the buffer held before ral_backward").  k_unet_fold now zeroes those floats in the launch it already makes.  The (1, 48)
     model, RA-LENet, ACDAE and DANet clear the whole buffer and always did.
  2. Header statements corrected, the library unchanged: ral_forward_begin also clears bn_sums[32, 64), and stage 0 of a U-Net
     training forward all 1280 doubles, not only the ranges named for them; ral_backward's "dx optional" does not hold for the
     U-Net, which refuses a dx.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import framed_util as fu
from ecg_denoise_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VP = C.c_void_p

# ---- the ledger ---------------------------------------------------------------------------------------------------------------
CASES = {}        # entry point -> the tests of this file that claim it (and assert that the proxy saw it)


def covers(*entries):
    def deco(fn):
        fn._entries = entries
        for e in entries:
            CASES.setdefault(e, []).append(fn.__name__)
        return fn
    return deco


# (entry point, argument index) -> why an argument typed c_void_p need not point into a framed payload
_HANDLE_FIRST = ("ral_destroy", "ral_bind", "ral_forward", "ral_forward_begin", "ral_forward_end", "ral_loss", "ral_forward_loss_means",
                 "ral_backward", "ral_backward_input", "ral_backward_begin", "ral_backward_input_begin", "ral_backward_input_end",
                 "ral_backward_end", "ral_unet_forward_stage", "ral_unet_forward_finish", "ral_unet_backward_start",
                 "ral_unet_backward_stage", "ral_unet_backward_finish", "ral_grad_bucket", "ral_grad_bucket_wait", "ral_adam_step",
                 "ral_debug_tensor", "ral_set_option", "ral_profile_select", "ral_profile_read", "ral_profile_timeline")
_NO_STREAM = ("ral_destroy", "ral_bind", "ral_grad_bucket", "ral_debug_tensor", "ral_set_option", "ral_profile_select",
              "ral_profile_read", "ral_profile_timeline", "ral_mix_draw", "ral_pe_table")
EXEMPT = {}
for _name, (_res, _args) in _lib._SIGS.items():
    if VP in _args:
        if _name in _HANDLE_FIRST:
            EXEMPT[(_name, 0)] = "the handle"
        if _name not in _NO_STREAM:
            EXEMPT[(_name, len(_args) - 1)] = "the stream"
EXEMPT.update({
    ("ral_pool_windows", 3): "host table (tab.ctypes.data)", ("ral_pool_emit", 2): "host table",
    ("ral_newrale_pool_front", 3): "host table", ("ral_newrale_pool_back", 3): "host table",
    ("ral_rate_pool", 3): "host table", ("ral_beat_pool", 3): "host table", ("ral_rhythm_pool", 3): "host table",
    ("ral_hrv_windows", 5): "host table", ("ral_arrhythmia_windows", 7): "host table",
    ("ral_mix_records", 6): "host array offsets", ("ral_mix_records", 7): "host array snr_db",
    ("ral_mix_batch", 9): "host thresholds cum (they travel as kernel arguments)",
    ("ral_mix_draw", 5): "host thresholds cum", ("ral_mix_draw", 10): "host out-parameter draw[4]",
    ("ral_mix_draw", 11): "host out-parameter snr_db",
    ("ral_pe_table", 2): "host out-parameter out_host",
})

# exports with a c_void_p that need no case here
LEDGER_EXEMPT = {
    "ral_create": "no device pointer (the handle comes back through a host out-parameter)",
    "ral_destroy": "the handle only",
    "ral_bind": "keeps pointers, launches nothing; every model case binds framed buffers through it",
    "ral_set_option": "the handle only",
    "ral_grad_bucket": "the handle and host out-parameters",
    "ral_grad_bucket_wait": "the handle and a stream",
    "ral_profile_select": "the handle only", "ral_profile_read": "the handle and host out-parameters",
    "ral_profile_timeline": "the handle and host out-parameters",
    "ral_debug_tensor": "returns a pointer into the handle's own workspace (out of scope)",
    "ral_mix_draw": "host arithmetic only: no device pointer is involved",
    "ral_pe_table": "writes a host table: no device pointer is involved",
}


# ---- helpers ------------------------------------------------------------------------------------------------------------------

def _vp(t):
    return VP(t.data_ptr()) if t is not None else VP(0)


def _stream():
    return VP(torch.cuda.current_stream().cuda_stream)


def _same_bits(a, b):
    if tuple(a.shape) != tuple(b.shape) or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    return torch.equal(a.contiguous().view(torch.uint8).cpu(), b.contiguous().view(torch.uint8).cpu())


def _rel(a, b):
    a, b = a.double().cpu().reshape(-1), b.double().cpu().reshape(-1)
    if a.numel() != b.numel():
        return float("inf")
    if b.numel() == 0:
        return 0.0
    n = b.norm().item()
    return ((a - b).norm().item() / n) if n > 0 else (a - b).abs().max().item()


def _poison(t):
    """fill a contiguous 4- or 8-byte tensor with the pattern word"""
    t.view(-1).view(torch.int32).fill_(fu.WORD)
    return t


class Abi:
    """one case's registry, proxy and switches"""

    def __init__(self, monkeypatch, claimed):
        self.reg = fu.Registry()
        self.real = _lib.lib()
        self.proxy = fu.AbiProxy(self.real, _lib._SIGS, self.reg, EXEMPT)
        self.mp, self.claimed = monkeypatch, claimed

    def on(self):
        self.mp.setattr(_lib, "_lib", self.proxy)

    def off(self):
        self.mp.setattr(_lib, "_lib", self.real)

    def F(self, t, name=None):
        """a framed copy of t on the device"""
        t = torch.as_tensor(t)
        return self.reg.like(t if t.is_cuda else t.to(DEV), name=name)

    def new(self, shape, dtype=torch.float32, fill=None, name=None):
        return self.reg.framed(shape, dtype, DEV, fill, name)

    def reframe(self, obj, *attrs):
        for k in attrs:
            setattr(obj, k, self.F(getattr(obj, k), name=f"{type(obj).__name__}.{k}"))

    def factories(self):
        return fu.framed_factories(self.reg, concat=True)

    def finish(self, written=()):
        torch.cuda.synchronize()
        self.reg.check_all()
        for name, t in (written.items() if isinstance(written, dict) else written):
            if t is not None:
                n = fu.unwritten(t)
                assert n == 0, f"{name}: {n} of {t.numel()} elements were never written"
        missing = set(self.claimed) - self.proxy.seen
        assert not missing, f"claimed but never called through the proxy: {sorted(missing)}"


@pytest.fixture
def abi(request, monkeypatch):
    a = Abi(monkeypatch, getattr(request.function, "_entries", ()))
    yield a
    a.off()


@pytest.fixture(autouse=True)
def _end_the_session_after_a_device_error():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # a fault leaves the context unusable: nothing more is started on the device
        pytest.exit(f"device error, the session ends here: {e}", returncode=3)


def fr(a, t):
    """t as this run takes it: a framed copy (a: the case's Abi) or an ordinary device tensor (a is None)"""
    t = torch.as_tensor(t)
    return a.F(t) if a is not None else t.to(DEV).contiguous()


def both(abi, fn, tol=None, partial=(), unchecked=()):
    """fn(None) on ordinary tensors, fn(abi) on framed ones with framed allocation and the proxy active -> (got, want), after the
    frame, pattern and result checks.  fn returns {name: tensor}, compared bit for bit; `tol`: {name: relative L2 bar} for the
    names that are not; `partial`: names whose pattern words are not counted; `unchecked`: names that are not compared"""
    want = fn(None)
    torch.cuda.synchronize()
    abi.on()
    with abi.factories():
        got = fn(abi)
        torch.cuda.synchronize()
    abi.off()
    abi.finish({k: v for k, v in got.items() if k not in partial})
    tol = tol or {}
    assert set(got) == set(want)
    for k in want:
        if k in unchecked:
            continue
        if want[k] is None:
            assert got[k] is None
        elif k in tol:
            e = _rel(got[k], want[k])
            assert e == e and e <= tol[k], f"{k}: relative L2 {e:.3e} > {tol[k]:.0e} against the run on ordinary tensors"
        else:
            assert _same_bits(got[k], want[k]), f"{k}: not the bits of the run on ordinary tensors"
    return got, want


# ---- the helper's own sensitivity (torch only, never a library kernel) -------------------------------------------------------------

def test_check_sees_one_element_past_the_payload():
    reg = fu.Registry()
    v = reg.framed((5, 3), torch.float32, DEV)
    e = reg.entry_of(v)
    reg.check(v)
    e.raw[e.off + e.nbytes:e.off + e.nbytes + 4].view(torch.float32).fill_(1.0)      # element [5, 0] of a (5, 3) tensor
    torch.cuda.synchronize()
    with pytest.raises(fu.FrameError, match=r"rear frame damaged, first damaged byte 0 byte\(s\) past the end"):
        reg.check(v)
    z = reg.framed((0,), torch.float64, DEV)                                         # zero length: the frames touch
    reg.check(z)
    assert fu.unwritten(v) == 15
    v[1, 1] = float("nan")
    assert fu.unwritten(v) == 14                                                    # a NaN result is not the pattern


def test_proxy_refuses_an_ordinary_tensor(abi):
    x = abi.new((4,), fill=1.0)
    plain = torch.zeros(4, device=DEV)
    abi.on()
    with pytest.raises(fu.FrameError, match=r"ral_wavelet_denoise: argument 1 "):
        _lib.lib().ral_wavelet_denoise(_vp(x), _vp(plain), 1, 4, 0.04, _stream())      # refused before the call is made
    abi.off()
    assert "ral_wavelet_denoise" not in abi.proxy.seen


def test_framed_factories_redirect_on_the_device_only(abi):
    with abi.factories():
        a = torch.empty(3, 5, dtype=torch.int32, device=DEV)
        b = torch.zeros((2, 2), device=torch.device(DEV))
        c = torch.full((4,), 7, dtype=torch.int64, device=DEV)
        d = torch.full_like(b, 2.0)
        e = torch.empty_like(a)
        h = torch.zeros(3)
    assert all(abi.reg.find(t.data_ptr()) is not None for t in (a, b, c, d, e)) and abi.reg.find(h.data_ptr()) is None
    assert fu.unwritten(a) == 15 and fu.unwritten(e) == 15 and (b == 0).all() and (c == 7).all() and (d == 2).all()
    assert a.data_ptr() % 512 == 0 and c.dtype == torch.int64 and d.dtype == torch.float32 and not h.is_cuda


# ---- model handles ----------------------------------------------------------------------------------------------------------------

def _model(kind, leads, L, max_batch, seed=11):
    from ecg_denoise_amd import ACDAE, DANet, RALENet, UNet
    if kind == "unet":
        return UNet(leads=leads, L=L, max_batch=max_batch, train=True, device=DEV, seed=seed)
    if kind == "acdae":
        return ACDAE(L=L, max_batch=max_batch, train=True, device=DEV, seed=seed)
    if kind == "danet":
        return DANet(L=L, max_batch=max_batch, train=True, device=DEV, seed=seed)
    return RALENet(kind, leads=leads, L=L, max_batch=max_batch, train=True, device=DEV, seed=seed)


def _xt(B, leads, L, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, leads, L, generator=g), torch.randn(B, leads, L, generator=g)


def _entries(m, buf):
    return {e["name"]: m.eng.view(buf, e) for e in m.eng.entries if e["kind"] == _lib.KIND_PARAM}


LR = 1e-3


def _cycle(a, kind, leads, L, B, max_batch, opts, after=None):
    """eval forward, forward_loss_means, ral_loss, backward with dx, adam_step, eval forward -> {name: tensor}.  `after`: the flat
    parameters and running statistics another run had after its step; they replace this run's own before the last eval forward,
    so that this forward can be compared bit for bit (the first Adam step moves every parameter by lr * g / (|g| + eps): where a
    gradient is rounding noise of atomic sums, its sign - and with it 2 lr of the parameter - differs from run to run)"""
    m = _model(kind, leads, L, max_batch)
    for k, v in opts.items():
        _lib.check(_lib.lib().ral_set_option(m.eng.h, k.encode(), v))
    x, t = _xt(B, leads, L)
    x, t = fr(a, x), fr(a, t)
    if a is not None:
        bufs = fu.frame_engine(m.eng, a.reg, a.real)
        assert bufs["bn_sums"].numel() == a.real.ral_bn_sums_doubles(C.byref(m.eng.cfg))
        _poison(bufs["grads"])               # "zeroed first": nothing of the old contents may survive in a parameter's gradient
    out = {}
    m.eval()
    out["y_eval0"] = m(x)
    m.train()
    y, loss, snr, rmse = m.forward_loss(x, t)
    out.update(y=y, means3=m._means, snr=snr, rmse=rmse, dy=m._dy)
    # the handle's own loss entry point on the same prediction: loss_sum accumulates into one double
    dy2, snr2, rmse2 = torch.empty_like(y), torch.empty_like(snr), torch.empty_like(rmse)
    loss_sum = torch.zeros(1, dtype=torch.float64, device=y.device)
    _lib.check(_lib.lib().ral_loss(m.eng.h, _vp(y), _vp(t), B, B, _vp(dy2), _vp(snr2), _vp(rmse2), _vp(loss_sum), _stream()))
    out.update(dy2=dy2, snr2=snr2, rmse2=rmse2, loss_sum=loss_sum)
    out["dx"] = m.backward(want_dx=kind != "unet")      # (the U-Net provides no input gradient: it refuses a dx)
    torch.cuda.synchronize()
    for k, g in _entries(m, m.eng.grads).items():
        out["grad:" + k] = g.clone()
        if a is not None:
            n = fu.unwritten(g)
            assert n == 0, f"grads[{k}]: {n} of {g.numel()} elements keep what the buffer held before ral_backward"
    if a is not None:
        n = fu.unwritten(m.eng.grads)
        assert n == 0, f"grads: {n} floats between the parameters keep what the buffer held before ral_backward (ral_adam_step reads them)"
    m.step(LR)
    torch.cuda.synchronize()
    out["params"], out["state"] = m.eng.params.clone(), m.eng.state.clone()
    if after is not None:
        m.eng.params.copy_(after[0])
        m.eng.state.copy_(after[1])
    m.eval()                                   # (tells the library that the parameters may have changed)
    out["y_eval1"] = m(x)
    torch.cuda.synchronize()
    out["_scratch64"] = m._loss_scratch
    return out


def _noise(g):
    """A bias in front of a batch-statistics BatchNorm (U-Net, DANet) and the key half of to_kv.bias (RA-LENet) have a gradient
    that is identically zero: what the kernels leave there is the rounding noise of their sums, different from run to run.  The
    suite's own line between the two is a norm of 1e-5 (tests/test_gpu_unet.py), and 1e-5 its bound on the noise
    (tests/test_gpu_danet.py)."""
    return g.double().norm().item() <= 1e-5

MODEL_CASES = [
    ("full", 2, 256, 3, 3, {}), ("nra", 1, 128, 5, 5, {}), ("mlp", 2, 320, 2, 2, {}), ("full", 2, 32, 2, 2, {}),
    ("full", 2, 256, 2, 4, {}),                                           # B < max_batch, y sized for B
    ("unet", 1, 48, 5, 5, {"unet_fused": 0}), ("unet", 1, 48, 5, 5, {"unet_fused": 1}),
    ("unet", 2, 256, 3, 3, {"unet_fused": 0}), ("unet", 2, 256, 3, 3, {"unet_fused": 1}),
    ("acdae", 2, 64, 3, 3, {}), ("danet", 2, 32, 5, 5, {}),               # zero-length bn_sums
]


@covers("ral_forward", "ral_forward_loss_means", "ral_loss", "ral_backward", "ral_adam_step")
@pytest.mark.parametrize("kind,leads,L,B,max_batch,opts", MODEL_CASES,
                         ids=[f"{c[0]}-{c[1]}x{c[2]}-B{c[3]}of{c[4]}" + "".join(f"-{k}{v}" for k, v in c[5].items()) for c in MODEL_CASES])
def test_model_handle(abi, kind, leads, L, B, max_batch, opts):
    if kind == "danet":      # (DANet counts its shared BatchNorms in a forward of its own: forward_loss is ral_forward + ral_loss_means there)
        abi.claimed = tuple(e for e in abi.claimed if e != "ral_forward_loss_means") + ("ral_loss_means",)
    want = _cycle(None, kind, leads, L, B, max_batch, opts)
    abi.on()
    with abi.factories():
        got = _cycle(abi, kind, leads, L, B, max_batch, opts, after=(want["params"], want["state"]))
    abi.off()
    s64 = got.pop("_scratch64")
    want.pop("_scratch64")
    abi.finish({k: got[k] for k in ("y_eval0", "y", "means3", "snr", "rmse", "dy", "dy2", "snr2", "rmse2", "dx", "y_eval1")})
    assert s64.numel() == 64 and (s64 == 0).all(), "scratch64 is left zero by every call"
    for k in ("y_eval0", "y_eval1"):
        assert _same_bits(got[k], want[k]), f"{k}: the eval forward is not the bits of the run on ordinary tensors"
    # one Adam step moves a parameter by at most lr (|g / (|g| + eps)| <= 1 at step 1), so two runs differ by at most 2 lr
    d = (got["params"].double() - want["params"].double()).abs().max().item()
    assert d == d and d <= 2 * LR * (1 + 1e-3), f"params after the step differ by {d:.3e} > 2 lr"
    for k in want:
        if k in ("y_eval0", "y_eval1", "params"):
            continue
        bar = 1e-4 if k.startswith("grad:") or k in ("dx", "state") else 1e-5
        if want[k] is None:
            assert got[k] is None, k
            continue
        if k.startswith("grad:") and _noise(want[k]):
            assert got[k].abs().max().item() < 1e-5, k
            continue
        e = _rel(got[k], want[k])
        assert e == e and e <= bar, f"{k}: relative L2 {e:.3e} > {bar:.0e} against the run on ordinary tensors"


def _newrale(a):
    from ecg_denoise_amd import NewRALE, RALENet
    inner = RALENet("full", leads=2, L=32, max_batch=2, train=True, device=DEV, seed=3)
    m = NewRALE(inner, seed=4)
    g = torch.Generator().manual_seed(8)
    x, t = fr(a, torch.randn(2, 12, 32, generator=g)), fr(a, torch.randn(2, 12, 32, generator=g))
    if a is not None:
        fu.frame_engine(inner.eng, a.reg, a.real)
        a.reframe(m, "params", "grads", "adam_m", "adam_v")       # the adapter's own flat buffers, 2216 floats each
        _poison(m.grads)                                           # NewRALE zeroes them itself before the four backward calls
    m.eval()
    out = {"y_eval": m(x)}
    m.train()
    r = m.train_step(x, t)
    torch.cuda.synchronize()
    out.update(pred=r["pred"], means3=m._means, snr=r["snr"], rmse=r["rmse"], dy=m._dy, grads=m.grads.clone(),
               params=m.params.clone(), adam_m=m.adam_m.clone(), adam_v=m.adam_v.clone())
    m.eval()
    out["y_eval_after"] = m(x)
    torch.cuda.synchronize()
    return out


@covers("ral_conv13_forward", "ral_conv13_backward", "ral_adam_flat", "ral_loss_means", "ral_backward_input", "ral_forward")
def test_newrale_handle(abi):
    """NewRALE at L = 32, B = 2 with its own flat buffer: an eval forward (bit for bit), one train step (four conv13 forwards,
    ral_loss_means, four conv13 backwards around ral_backward_input, ral_adam_flat) and an eval forward after it"""
    got, want = both(abi, _newrale, tol={k: 1e-4 for k in ("grads", "adam_m", "adam_v")} |
                     {k: 1e-5 for k in ("pred", "means3", "snr", "rmse", "dy")}, unchecked=("params", "y_eval_after"))
    d = (got["params"].double() - want["params"].double()).abs().max().item()
    assert d == d and d <= 2 * LR * (1 + 1e-3), f"adapter parameters after the step differ by {d:.3e} > 2 lr (one Adam step moves each by at most lr)"


def _blocks_changed(before, after, width=64):
    b = before.view(torch.int64).cpu().reshape(-1, width)
    a = after.view(torch.int64).cpu().reshape(-1, width)
    return set(torch.nonzero((a != b).any(dim=1)).reshape(-1).tolist())


@covers("ral_forward_begin", "ral_forward_end", "ral_backward_begin", "ral_backward_end", "ral_backward_input",
        "ral_backward_input_begin", "ral_backward_input_end")
def test_split_ralenet(abi):
    """The data-parallel cut of RA-LENet ("full", 2, 256, B = 3) on one process (global_windows = B).  bn_sums is 64 doubles,
    pattern-filled before the first call: forward_begin leaves sums in [0, 32) (and may only clear [32, 64)), forward_end changes
    nothing, the backward begins leave sums in [32, 64) and do not touch [0, 32), the ends change nothing."""
    kind, leads, L, B = "full", 2, 256, 3
    xh, th = _xt(B, leads, L)
    ref = _model(kind, leads, L, B)                            # the unsplit calls on ordinary tensors
    ref.train()
    y_ref, _, _, _ = ref.forward_loss(xh.to(DEV), th.to(DEV))
    dx_ref = ref.backward(want_dx=True)
    g_ref = {k: v.clone() for k, v in _entries(ref, ref.eng.grads).items()}
    dy_ref = ref._dy.clone()
    torch.cuda.synchronize()

    m = _model(kind, leads, L, B)
    bufs = fu.frame_engine(m.eng, abi.reg, abi.real)
    sums = _poison(bufs["bn_sums"])
    assert sums.numel() == 64
    x, dy = abi.F(xh), abi.F(dy_ref)
    y, dx, dx_in, dx_in2 = (abi.new((B, leads, L)) for _ in range(4))
    lib, h, snap = abi.proxy, m.eng.h, lambda: (torch.cuda.synchronize(), sums.clone())[1]
    abi.on()
    m.train()
    s0 = snap()
    _lib.check(lib.ral_forward_begin(h, _vp(x), B, _stream()))
    s1 = snap()
    _lib.check(lib.ral_forward_end(h, _vp(y), B, B, _stream()))
    s2 = snap()
    _poison(bufs["grads"])
    _lib.check(lib.ral_backward_begin(h, _vp(dy), B, _stream()))
    s3 = snap()
    _lib.check(lib.ral_backward_end(h, _vp(dx), B, B, _stream()))
    s4 = snap()
    grads = {k: v.clone() for k, v in _entries(m, m.eng.grads).items()}
    _lib.check(lib.ral_backward_input_begin(h, _vp(dy), B, _stream()))
    s5 = snap()
    _lib.check(lib.ral_backward_input_end(h, _vp(dx_in), B, B, _stream()))
    s6 = snap()
    _lib.check(lib.ral_backward_input(h, _vp(dy), _vp(dx_in2), B, _stream()))
    abi.off()
    abi.finish({"y": y, "dx": dx, "dx_in": dx_in, "dx_in2": dx_in2})
    assert fu.unwritten(s0) == 64
    assert fu.unwritten(s1[:32]) == 0, "forward_begin leaves its sums in bn_sums[0, 32)"
    assert fu.unwritten(s1[32:]) == 32 or (s1[32:] == 0).all(), "forward_begin may leave [32, 64) alone or clear it, nothing else"
    assert _same_bits(s2, s1), "forward_end changed bn_sums"
    assert _same_bits(s3[:32], s2[:32]) and fu.unwritten(s3[32:]) == 0, "backward_begin writes [32, 64) and nothing else"
    assert _same_bits(s4, s3), "backward_end changed bn_sums"
    assert _same_bits(s5[:32], s4[:32]) and _same_bits(s6, s5), "the input-gradient pair writes [32, 64) in its begin only"
    for k, g in grads.items():
        assert fu.unwritten(g) == 0, k
        if _noise(g_ref[k]):
            assert g.abs().max().item() < 1e-5, k
        else:
            assert _rel(g, g_ref[k]) <= 1e-4, k
    assert _rel(y, y_ref) <= 1e-5
    for name, t in (("dx", dx), ("dx_in", dx_in), ("dx_in2", dx_in2)):
        assert _rel(t, dx_ref) <= 1e-4, name


@covers("ral_unet_forward_stage", "ral_unet_forward_finish", "ral_unet_backward_start", "ral_unet_backward_stage",
        "ral_unet_backward_finish")
def test_split_unet(abi):
    """The U-Net (2, 256, B = 3) one stage at a time.  bn_sums is 10 x 128 doubles, BatchNorm bn owning [128 bn, 128 bn + 64)
    (forward sums) and [128 bn + 64, 128 bn + 128) (backward sums); pattern-filled before stage 0, which clears all of it.
    A forward stage si > 0 changes its own BatchNorm's forward half at most, forward_finish no backward half; the backward calls
    change backward halves only, ral_unet_backward_start that of BatchNorm 9 only."""
    leads, L, B = 2, 256, 3
    xh, th = _xt(B, leads, L)
    ref = _model("unet", leads, L, B)
    ref.train()
    y_ref, _, _, _ = ref.forward_loss(xh.to(DEV), th.to(DEV))
    dy_ref = ref._dy.clone()
    ref.backward(dy_ref)
    g_ref = {k: v.clone() for k, v in _entries(ref, ref.eng.grads).items()}
    torch.cuda.synchronize()

    m = _model("unet", leads, L, B)
    bufs = fu.frame_engine(m.eng, abi.reg, abi.real)
    sums = _poison(bufs["bn_sums"])
    assert sums.numel() == 1280
    x, dy, y = abi.F(xh), abi.F(dy_ref), abi.new((B, leads, L))
    lib, h, snap = abi.proxy, m.eng.h, lambda: (torch.cuda.synchronize(), sums.clone())[1]
    abi.on()
    m.train()
    log, prev = [], snap()

    def step(name, allowed):
        nonlocal prev
        cur = snap()
        ch = _blocks_changed(prev, cur)
        log.append((name, sorted(ch)))
        prev = cur
        assert allowed is None or ch <= allowed, f"{name} changed the 64-double blocks {sorted(ch)} of bn_sums, documented: {sorted(allowed)}"

    for si in range(11):
        _lib.check(lib.ral_unet_forward_stage(h, _vp(x), B, 1, si, B, _stream()))
        bn = abi.real.ral_unet_stage_bn(si)
        step(f"forward_stage({si})", None if si == 0 else ({2 * bn} if bn >= 0 else set()))
        if bn >= 0:
            assert fu.unwritten(prev[128 * bn:128 * bn + 64]) == 0, f"forward_stage({si}) leaves its sums in BatchNorm {bn}'s forward half"
    _lib.check(lib.ral_unet_forward_finish(h, _vp(y), B, 1, B, _stream()))
    step("forward_finish", {2 * k for k in range(10)})
    _poison(bufs["grads"])
    _lib.check(lib.ral_unet_backward_start(h, _vp(dy), B, B, _stream()))
    step("backward_start", {2 * 9 + 1})
    for si in range(10, -1, -1):
        _lib.check(lib.ral_unet_backward_stage(h, B, si, B, _stream()))
        step(f"backward_stage({si})", {2 * k + 1 for k in range(10)})
    _lib.check(lib.ral_unet_backward_finish(h, B, B, _stream()))
    step("backward_finish", {2 * k + 1 for k in range(10)})
    abi.off()
    print("bn_sums blocks changed per call:", log)
    abi.finish({"y": y})
    assert _rel(y, y_ref) <= 1e-5
    for k, g in _entries(m, m.eng.grads).items():
        assert fu.unwritten(g) == 0, k
        if _noise(g_ref[k]):
            assert g.abs().max().item() < 1e-5, k
        else:
            assert _rel(g, g_ref[k]) <= 1e-4, k


# ---- stateless operators, raw ABI ---------------------------------------------------------------------------------------------------

def _alloc(a):
    """-> (empty, zeros): allocators of this run, pattern-filled framed payloads or ordinary tensors"""
    if a is None:
        return (lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=DEV),
                lambda shape, dtype=torch.float32, fill=0: torch.full(shape, fill, dtype=dtype, device=DEV))
    return (lambda shape, dtype=torch.float32: a.new(shape, dtype),
            lambda shape, dtype=torch.float32, fill=0: a.new(shape, dtype, fill=fill))


def _raw(abi, fn, **kw):
    """`both` for a case that calls the ABI itself: the library is `_lib.lib()` in both runs"""
    return both(abi, fn, **kw)


ATTN_SHAPES = [(32, 2, 24, 3), (64, 16, 4, 5), (64, 16, 0, 5), (128, 8, 8, 3), (256, 4, 16, 3), (512, 2, 32, 2), (48, 8, 8, 3),
               (288, 2, 0, 3), (1024, 1, 0, 1)]


@covers("ral_attention_forward", "ral_attention_backward")
@pytest.mark.parametrize("N,H,Len,B", ATTN_SHAPES)
def test_attention_operator(abi, N, H, Len, B):
    """scratch at exactly ral_attention_backward_scratch_floats floats, pattern-filled (the (B, 2, H, 64) tail nothing reads
    included); gtable is accumulated into, from 0.25 everywhere"""
    g = torch.Generator().manual_seed(N + Len)
    qkv = torch.randn(B, 3 * H, N, 4, generator=g)
    qkv[:, :H] *= 0.5
    table = 0.5 * torch.randn(2 * Len - 1, H, generator=g) if Len else None
    do = torch.randn(B, H, N, 4, generator=g)

    def fn(a):
        E, Z = _alloc(a)
        L = _lib.lib()
        qd, dod, td = fr(a, qkv), fr(a, do), (fr(a, table) if Len else None)
        o, lse, dqkv = E((B, H, N, 4)), E((B, H, N)), E((B, 3 * H, N, 4))
        gt = Z((2 * Len - 1, H), fill=0.25) if Len else None
        _lib.check(L.ral_attention_forward(_vp(qd), _vp(o), _vp(lse), _vp(td), N, H, Len, B, _stream()))
        ns = L.ral_attention_backward_scratch_floats(N, H, Len, int(bool(Len)), B)
        assert ns >= 0, L.ral_last_error()
        scratch = E((ns,)) if ns else None
        _lib.check(L.ral_attention_backward(_vp(qd), _vp(o), _vp(dod), _vp(lse), _vp(td), _vp(gt), _vp(dqkv), _vp(scratch), ns,
                                            N, H, Len, B, _stream()))
        torch.cuda.synchronize()
        assert _same_bits(qd, qkv.to(DEV)) and _same_bits(dod, do.to(DEV)), "an input changed"
        return {"o": o, "lse": lse, "dqkv": dqkv, "gtable": gt}

    _raw(abi, fn, tol={"dqkv": 2e-5, "gtable": 2e-5}, partial=("gtable",))


@pytest.mark.parametrize("opts", ["attn_f16=0", "attn_bwd_m=0,attn_bwd_mh=0,attn_bwd_w=0,attn_fwd_w=0,attn_fwd_h=0"])
def test_attention_operator_every_kernel_choice(opts):
    """the attention cases again in a process of its own per option string (tests/conftest.py applies RAL_TEST_OPTIONS): the
    two-sweep and per-workgroup-partial kernels"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                        "test_attention_operator and not every_kernel_choice", "-p", "no:cacheprovider"],
                       env=dict(os.environ, RAL_TEST_OPTIONS=opts), cwd=root, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, f"RAL_TEST_OPTIONS={opts}\n{p.stdout[-3000:]}\n{p.stderr[-2000:]}"
    assert f"{len(ATTN_SHAPES)} passed" in p.stdout, p.stdout[-1000:]


@covers("ral_loss_flat", "ral_loss_mean", "ral_loss_means")
@pytest.mark.parametrize("B,n", [(5, 1022), (5, 1028), (2049, 8), (1, 4)])
def test_loss_operators(abi, B, n):
    """loss_sum and loss_mean are 1 double, scratch2 exactly 2, means3 exactly 3, scratch64 exactly 64.  The per-window outputs
    and dy are compared bit for bit; the sums over windows come out of double atomics, whose order moves the last bits: B
    additions of positive terms differ by at most B * 2^-53 relative, far inside 1e-12."""
    g = torch.Generator().manual_seed(B + n)
    pred, tgt = torch.randn(B, n, generator=g), torch.randn(B, n, generator=g)

    def fn(a):
        E, Z = _alloc(a)
        L, out = _lib.lib(), {}
        p, t = fr(a, pred), fr(a, tgt)
        D = torch.float64
        for name in ("flat", "mean", "means"):
            dy, snr, rmse = E((B, n)), E((B,)), E((B,))
            if name == "flat":
                acc = Z((1,), D)
                _lib.check(L.ral_loss_flat(_vp(p), _vp(t), n, B, B, _vp(dy), _vp(snr), _vp(rmse), _vp(acc), _stream()))
            elif name == "mean":
                acc, sc = E((1,), D), Z((2,), D)
                _lib.check(L.ral_loss_mean(_vp(p), _vp(t), n, B, B, _vp(dy), _vp(snr), _vp(rmse), _vp(acc), _vp(sc), _stream()))
                _lib.check(L.ral_loss_mean(_vp(p), _vp(t), n, B, B, _vp(dy), _vp(snr), _vp(rmse), _vp(acc), _vp(sc), _stream()))
            else:
                acc, sc = E((3,), D), Z((64,), D)
                _lib.check(L.ral_loss_means(_vp(p), _vp(t), n, B, B, _vp(dy), _vp(snr), _vp(rmse), _vp(acc), _vp(sc), _stream()))
                _lib.check(L.ral_loss_means(_vp(p), _vp(t), n, B, B, _vp(dy), _vp(snr), _vp(rmse), _vp(acc), _vp(sc), _stream()))
            torch.cuda.synchronize()
            if name != "flat":
                assert (sc == 0).all(), f"loss_{name}: the scratch is left zero by every call"
            out.update({f"{name}:dy": dy, f"{name}:snr": snr, f"{name}:rmse": rmse, f"{name}:sum": acc})
        assert _same_bits(p, pred.to(DEV)) and _same_bits(t, tgt.to(DEV)), "an input changed"
        return out

    got, _ = _raw(abi, fn, tol={"flat:sum": 1e-12, "mean:sum": 1e-12, "means:sum": 1e-12})
    ref = ((pred.double() - tgt.double()) ** 2).mean(1).sum().item()
    assert abs(got["flat:sum"].item() - ref) <= 1e-5 * ref and abs(got["mean:sum"].item() * B - ref) <= 1e-5 * ref


@covers("ral_adam_flat")
@pytest.mark.parametrize("n", [4, 1028, 8192 * 256 * 4 + 4])
def test_adam_flat(abi, n):
    """n = 4 and 1028: the float4 path with and without whole vectors beyond the first; 8192 * 256 * 4 + 4: the first length the
    capped grid strides over"""
    g = torch.Generator().manual_seed(n % 1000)
    p0, g0, m0 = torch.randn(n, generator=g), torch.randn(n, generator=g), 0.1 * torch.randn(n, generator=g)
    v0 = 0.01 * torch.rand(n, generator=g)

    def fn(a):
        p, gr, m, v = fr(a, p0), fr(a, g0), fr(a, m0), fr(a, v0)
        _lib.check(_lib.lib().ral_adam_flat(_vp(p), _vp(gr), _vp(m), _vp(v), n, 1e-3, 0.9, 0.999, 1e-8, 3, 0.5, _stream()))
        torch.cuda.synchronize()
        assert _same_bits(gr, g0.to(DEV)), "the gradient is an input"
        return {"p": p, "m": m, "v": v}

    got, _ = _raw(abi, fn)
    mh = 0.9 * m0.double() + 0.1 * 0.5 * g0.double()
    assert _rel(got["m"], mh) < 1e-6


@covers("ral_conv13_forward", "ral_conv13_backward")
@pytest.mark.parametrize("cin,cout,L,B", [(12, 6, 16, 3), (6, 2, 16, 3), (2, 6, 16, 3), (6, 12, 16, 3), (12, 6, 1000, 3), (6, 2, 1000, 3),
                                          (2, 6, 1000, 3), (6, 12, 1000, 3), (1, 1, 1, 3)])
def test_conv13_operators(abi, cin, cout, L, B):
    """the adapter's four channel pairs at L = 16 and 1000, and cin = cout = 1 at L = 1; gw and gb are accumulated into, from 0.5
    everywhere (1e-4: the bar of the parameter gradients)"""
    g = torch.Generator().manual_seed(cin * 100 + cout + L)
    x0, w0, b0 = torch.randn(B, cin, L, generator=g), 0.2 * torch.randn(cout, cin, 13, generator=g), torch.randn(cout, generator=g)
    dy0 = torch.randn(B, cout, L, generator=g)

    def fn(a):
        E, Z = _alloc(a)
        lib = _lib.lib()
        x, w, b, dy = fr(a, x0), fr(a, w0), fr(a, b0), fr(a, dy0)
        y, dx = E((B, cout, L)), E((B, cin, L))
        gw, gb = Z((cout, cin, 13), fill=0.5), Z((cout,), fill=0.5)
        _lib.check(lib.ral_conv13_forward(_vp(x), _vp(w), _vp(b), _vp(y), B, cin, cout, L, 1, _stream()))
        _lib.check(lib.ral_conv13_backward(_vp(x), _vp(y), _vp(dy), _vp(w), _vp(gw), _vp(gb), _vp(dx), B, cin, cout, L, 1, _stream()))
        torch.cuda.synchronize()
        assert all(_same_bits(u, v.to(DEV)) for u, v in ((x, x0), (w, w0), (b, b0), (dy, dy0))), "an input changed"
        return {"y": y, "dx": dx, "gw": gw, "gb": gb}

    got, _ = _raw(abi, fn, tol={"dx": 1e-5, "gw": 1e-4, "gb": 1e-4})
    ref = torch.nn.functional.leaky_relu(torch.nn.functional.conv1d(x0.double(), w0.double(), b0.double(), padding=6), 0.01)
    assert _rel(got["y"], ref) < 1e-5


@covers("ral_wavelet_denoise")
@pytest.mark.parametrize("L", [14, 30, 1000, 8192])
def test_wavelet_denoise(abi, L):
    """rows = 3; L = 14 has no level at all, 30 the first odd-length band, 8192 is the longest record"""
    x0 = torch.randn(3, L, generator=torch.Generator().manual_seed(L))

    def fn(a):
        E, _ = _alloc(a)
        x, y = fr(a, x0), E((3, L))
        _lib.check(_lib.lib().ral_wavelet_denoise(_vp(x), _vp(y), 3, L, 0.04, _stream()))
        torch.cuda.synchronize()
        assert _same_bits(x, x0.to(DEV)), "the input changed"
        return {"y": y}

    _raw(abi, fn)


@covers("ral_fft_denoise")
@pytest.mark.parametrize("groups,rows,L", [(2, 2, 18), (2, 2, 1000), (2, 2, 17), (2, 2, 375), (2, 12, 8192)])
def test_fft_denoise(abi, groups, rows, L):
    """2 groups x 2 rows at a mixed-radix and a direct length each, and 2 x 12 x 8192, which takes two launches and the scratch of
    exactly ral_fft_denoise_scratch_bytes bytes"""
    x0 = torch.randn(groups, rows, L, generator=torch.Generator().manual_seed(L))

    def fn(a):
        E, _ = _alloc(a)
        lib = _lib.lib()
        nbytes = lib.ral_fft_denoise_scratch_bytes(groups, rows, L)
        assert nbytes >= 0 and (nbytes > 0) == (L == 8192), nbytes
        x, y, kept = fr(a, x0), E((groups, rows, L)), E((groups,), torch.int32)
        scratch = E((nbytes,), torch.uint8) if nbytes else None
        _lib.check(lib.ral_fft_denoise(_vp(x), _vp(y), _vp(kept), groups, rows, L, 0.04, _vp(scratch), _stream()))
        torch.cuda.synchronize()
        assert _same_bits(x, x0.to(DEV)), "the input changed"
        return {"y": y, "kept": kept}

    _raw(abi, fn)


@covers("ral_prep_windows")
@pytest.mark.parametrize("leads", [1, 2])
def test_prep_windows(abi, leads):
    """sums is exactly 2 * leads + 1 doubles of scratch, pattern-filled.  The statistics are double sums whose order may move
    their last bits: 1e-6 relative L2, ten fp32 roundings."""
    T, L = 4 * 64, 64
    g = torch.Generator().manual_seed(leads)
    sig0, noi0 = 1000 + 200 * torch.randn(T, leads, generator=g), 30 * torch.randn(T, leads, generator=g)

    def fn(a):
        E, _ = _alloc(a)
        sig, noi = fr(a, sig0), fr(a, noi0)
        sums, noisy, clean = E((2 * leads + 1,), torch.float64), E((T // L, leads, L)), E((T // L, leads, L))
        _lib.check(_lib.lib().ral_prep_windows(_vp(sig), _vp(noi), T, leads, L, 6.0, _vp(sums), _vp(noisy), _vp(clean), _stream()))
        torch.cuda.synchronize()
        return {"noisy": noisy, "clean": clean}

    got, _ = _raw(abi, fn, tol={"noisy": 1e-6, "clean": 1e-6})
    z = (sig0.double() - sig0.double().mean(0)) / sig0.double().std(0, unbiased=False)
    assert _rel(got["clean"], z.T.reshape(leads, T // L, L).permute(1, 0, 2)) < 1e-5


@covers("ral_stream_windows", "ral_stream_stitch")
def test_stream_windows_and_stitch(abi):
    """R = 2, leads = 2, L = 64, hop = 48, T = 200: four windows per record, the last right-aligned.  A call for windows [1, 4)
    writes a win of exactly three windows and their twelve stats values; the other stats entries keep the pattern."""
    R, leads, L, hop, T = 2, 2, 64, 48, 200
    n = (T - L) // hop + 1 + (1 if (T - L) % hop else 0)
    rec0 = torch.randn(R, leads, T, generator=torch.Generator().manual_seed(1)) * 3 + 1

    def fn(a):
        E, _ = _alloc(a)
        lib = _lib.lib()
        rec = fr(a, rec0)
        win, stats, out = E((R * n, leads, L)), E((R * n * leads * 2,)), E((R, leads, T))
        _lib.check(lib.ral_stream_windows(_vp(rec), R, T, leads, L, hop, 0, R * n, _vp(win), _vp(stats), _stream()))
        _lib.check(lib.ral_stream_stitch(_vp(win), _vp(stats), R, T, leads, L, hop, _vp(out), _stream()))
        win3, stats3 = E((3, leads, L)), E((R * n * leads * 2,))
        _lib.check(lib.ral_stream_windows(_vp(rec), R, T, leads, L, hop, 1, 3, _vp(win3), _vp(stats3), _stream()))
        torch.cuda.synchronize()
        assert _same_bits(win3, win[1:4]) and _same_bits(stats3[leads * 2:4 * leads * 2], stats[leads * 2:4 * leads * 2])
        if a is not None:
            assert fu.unwritten(stats3) == (R * n - 3) * leads * 2, "a partial call writes the stats of its own windows only"
        return {"win": win, "stats": stats, "out": out, "win3": win3}

    got, _ = _raw(abi, fn)
    assert _rel(got["out"], rec0) < 1e-5          # z-score, de-normalise and stitch give the record back


def _exact_bytes(E, nbytes):
    """a scratch of exactly nbytes, rounded up only to the 8-byte alignment the header demands"""
    return E(((nbytes + 7) // 8 * 8,), torch.uint8)


@covers("ral_mix_records", "ral_score_records")
def test_mix_and_score_records(abi):
    """R = 3, leads = 2, T = 1001, W = 250 (a trailing partial tile), the scratch at the queried bytes"""
    R, leads, T, Tn, W = 3, 2, 1001, 1500, 250
    g = torch.Generator().manual_seed(2)
    rec0, noi0 = 1000 + 100 * torch.randn(R, leads, T, generator=g), torch.randn(leads, Tn, generator=g)
    off, snr = np.array([0, 250, Tn - T], dtype=np.int64), np.array([-3.0, 0.0, 6.0])

    def fn(a):
        E, _ = _alloc(a)
        lib, D = _lib.lib(), torch.float64
        rec, noi = fr(a, rec0), fr(a, noi0)
        nb = lib.ral_mix_records_scratch_bytes(R, leads, T)
        assert nb > 0
        sc, noisy, clean = _exact_bytes(E, nb), E((R, leads, T)), E((R, leads, T))
        _lib.check(lib.ral_mix_records(_vp(rec), _vp(noi), R, leads, T, Tn, off.ctypes.data, snr.ctypes.data, _vp(sc), _vp(noisy),
                                       _vp(clean), _stream()))
        nb2 = lib.ral_score_records_scratch_bytes(R, leads, T, W)
        assert nb2 > 0
        sc2 = _exact_bytes(E, nb2)
        pl, pr, pw, wm = E((R, leads, 4), D), E((R, 4), D), E((R, T // W, 4), D), E((R + 1, 4), D)
        _lib.check(lib.ral_score_records(_vp(clean), _vp(noisy), _vp(noisy), R, leads, T, W, _vp(sc2), _vp(pl), _vp(pr), _vp(pw),
                                         _vp(wm), _stream()))
        torch.cuda.synchronize()
        return {"noisy": noisy, "clean": clean, "per_lead": pl, "per_record": pr, "per_window": pw, "window_mean": wm}

    got, _ = _raw(abi, fn)
    assert (got["per_record"][:, 0].cpu() - torch.from_numpy(snr)).abs().max() < 1e-3       # the "in" SNR is the one asked for


def _ecg(i):
    import beat_util
    return torch.from_numpy(beat_util.inputs()[i][1])


@covers("ral_beat_records")
def test_beat_records_exact_scratch(abi):
    """ral_beat_records at exactly ral_beat_records_scratch_bytes (rounded up to 8 only; BeatDetector adds a word), cap as the
    header defines it, against BeatDetector.detect on ordinary tensors"""
    from ecg_denoise_amd.beats import BeatDetector
    x0 = _ecg(0)                                            # (4, 2, 1440), clean
    R, leads, T = x0.shape
    det = BeatDetector(device=DEV)
    want = det.detect(x0.to(DEV))
    d, cap = det.det, det.cap(T)
    x, bank = abi.F(x0), abi.F(torch.from_numpy(d.bank_host))
    nb = abi.real.ral_beat_records_scratch_bytes(R, leads, T, d.geom)
    assert nb > 0
    E, _ = _alloc(abi)
    scratch, peaks, count = _exact_bytes(E, nb), E((R, cap), torch.int32), E((R,), torch.int32)
    abi.on()
    _lib.check(_lib.lib().ral_beat_records(_vp(x), R, leads, T, d.geom, _vp(bank), d.bank_host.size, _vp(scratch), scratch.numel(),
                                           _vp(peaks), cap, _vp(count), _stream()))
    abi.off()
    abi.finish({"peaks": peaks, "count": count})
    assert _same_bits(peaks, want.peaks) and _same_bits(count, want.count) and int(count.min()) >= 1


# ---- through the wrappers, framed allocation active ---------------------------------------------------------------------------------------

def _eval_model(kind="nra", leads=2, L=64, max_batch=8):
    from ecg_denoise_amd import RALENet
    return RALENet(kind, leads=leads, L=L, max_batch=max_batch, train=False, device=DEV, seed=21)


def _chunks(T, sizes):
    o = 0
    for c in sizes:
        yield o, min(o + c, T)
        o += c


@covers("ral_live_windows", "ral_live_emit", "ral_forward")
def test_live_pair(abi):
    """LiveDenoiser, S = 2 streams of 2 leads, L = 64, hop = 48, chunks of 96, a last chunk of 37: both histories hold the pattern
    when the streams start (positions below sample 0 are never read); last_y and last_stats are present in every push"""
    from ecg_denoise_amd.infer import LiveDenoiser
    rec = torch.randn(2, 2, 3 * 96 + 37, generator=torch.Generator().manual_seed(3))

    def fn(a):
        ld = LiveDenoiser(_eval_model(), streams=2, chunk=96, overlap=16, use_graph=False)
        if a is not None:
            _poison(ld.hist[0]), _poison(ld.hist[1])
        out = {}
        for i in range(3):
            out[f"push{i}"] = ld.push(rec[:, :, 96 * i:96 * (i + 1)], copy=True)
        out["flush"] = ld.flush(rec[:, :, 288:])
        torch.cuda.synchronize()
        return out

    got, _ = both(abi, fn)
    assert sum(v.shape[2] for v in got.values()) == rec.shape[2]


@covers("ral_pool_windows", "ral_pool_emit", "ral_forward")
def test_pool_pair(abi):
    """LivePool, capacity 3, L = 64, hop = 48: a call with a kept row and a closing row (from_last: the kept window emitted at
    close), both history planes pattern-filled before the streams open"""
    from ecg_denoise_amd.infer import LivePool
    g = torch.Generator().manual_seed(4)
    r0, r1 = torch.randn(2, 230, generator=g), torch.randn(2, 112, generator=g)

    def fn(a):
        pool = LivePool(_eval_model(), capacity=3, overlap=16)
        if a is not None:
            _poison(pool.hist)
        s0, s1 = pool.open(), pool.open()
        out = {}
        o = pool.push({s0: r0[:, :100], s1: r1[:, :112]})
        out["a0"], out["a1"] = o[s0], o[s1]
        o = pool.push({s0: r0[:, 100:150]}, close=(s1,))             # s0 stays open (kept row), s1 closes without a chunk
        out["b0"], out["b1"] = o[s0], o[s1]
        out["n0"] = pool.push({s0: r0[:, 150:155]})[s0]              # completes no window: the call only writes the next history
        out["c0"] = pool.close(s0, r0[:, 155:])
        torch.cuda.synchronize()
        return out

    got, _ = both(abi, fn)
    assert got["n0"].shape[1] == 0 and got["a1"].shape[1] + got["b1"].shape[1] == 112
    assert got["a0"].shape[1] + got["b0"].shape[1] + got["c0"].shape[1] == 230


def _newrale_eval(a):
    from ecg_denoise_amd import NewRALE, RALENet
    inner = RALENet("full", leads=2, L=32, max_batch=4, train=False, device=DEV, seed=31)
    m = NewRALE(inner, seed=32)
    if a is not None:
        a.reframe(m, "params")
    return m.eval()


@covers("ral_newrale_stream_front", "ral_newrale_stream_back", "ral_newrale_live_front", "ral_newrale_live_back",
        "ral_newrale_pool_front", "ral_newrale_pool_back", "ral_stream_windows", "ral_stream_stitch", "ral_forward")
def test_twelve_lead_stream_live_and_pool(abi):
    """NewRALE around RA-LENet ("full", 2, 32), overlap 8 (hop 24): StreamingDenoiser on 2 records of 100 samples in batches of 4
    windows, NewRALELiveDenoiser (chunks of 48, a last chunk of 11) and NewRALELivePool (a kept and a closing row), histories
    pattern-filled; and the 2-lead StreamingDenoiser through its wrapper"""
    from ecg_denoise_amd.infer import NewRALELiveDenoiser, NewRALELivePool, StreamingDenoiser
    g = torch.Generator().manual_seed(6)
    rec, rec2 = torch.randn(2, 12, 107, generator=g), torch.randn(2, 2, 200, generator=g)

    def fn(a):
        out = {}
        m = _newrale_eval(a)
        out["stream"] = StreamingDenoiser(m, batch=4, overlap=8, use_graph=False).denoise(rec[:, :, :100].to(DEV))
        ld = NewRALELiveDenoiser(m, streams=2, chunk=48, overlap=8, use_graph=False)
        pool = NewRALELivePool(m, capacity=3, overlap=8)
        if a is not None:
            _poison(ld.hist[0]), _poison(ld.hist[1]), _poison(pool.hist)
        out["push0"], out["push1"] = ld.push(rec[:, :, :48]), ld.push(rec[:, :, 48:96])
        out["flush"] = ld.flush(rec[:, :, 96:])
        s0, s1 = pool.open(), pool.open()
        o = pool.push({s0: rec[0, :, :50], s1: rec[1, :, :40]})
        out["a0"], out["a1"] = o[s0], o[s1]
        o = pool.push({s0: rec[0, :, 50:80]}, close=(s1,))
        out["b0"], out["b1"] = o[s0], o[s1]
        out["n0"] = pool.push({s0: rec[0, :, 80:83]})[s0]            # completes no window: the call only writes the next history
        out["c0"] = pool.close(s0, rec[0, :, 83:])
        out["stream2"] = StreamingDenoiser(_eval_model(), batch=3, overlap=16, use_graph=False).denoise(rec2.to(DEV))
        torch.cuda.synchronize()
        return out

    got, _ = both(abi, fn)
    assert sum(got[k].shape[2] for k in ("push0", "push1", "flush")) == 107
    assert got["n0"].shape[1] == 0 and got["a0"].shape[1] + got["b0"].shape[1] + got["c0"].shape[1] == 107


@covers("ral_mix_batch")
def test_mix_batch(abi):
    """NoiseMixSampler on augment_util's smallest case: a drawn batch and one with given rows, one of them outside the bank"""
    import augment_util
    from ecg_denoise_amd.augment import NoiseMixSampler
    bank, noise = augment_util.make_case(5, 2, 70, 3, 90, seed=9)

    def fn(a):
        s = NoiseMixSampler(bank, list(noise), L=64, seed=77, device=DEV)
        s._upload()
        if a is not None:
            a.reframe(s, "_bank", "_noise")
        b1 = s.batch(5)
        b2 = s.batch(3, rows=fr(a, torch.tensor([4, 0, 7], dtype=torch.int64)))
        torch.cuda.synchronize()
        return {"noisy1": b1.noisy, "clean1": b1.clean, "row1": b1.row, "snr1": b1.snr_db, "noisy2": b2.noisy, "clean2": b2.clean,
                "row2": b2.row, "kind2": b2.kind, "snr2": b2.snr_db}

    got, _ = both(abi, fn)
    assert got["row2"].tolist() == [4, 0, -1] and torch.isnan(got["noisy2"][2]).all()


@covers("ral_rate_records", "ral_rate_pool")
def test_rate_records_and_pool(abi):
    """Resampler and ResamplerPool 500 -> 360 Hz on rate_util's ADC-like records (2 leads, 700 samples): a kept row, a closing row
    with and one without a chunk; both history planes pattern-filled (whatever the slot held before is never read)"""
    import rate_util
    from ecg_denoise_amd.rate import Resampler, ResamplerPool
    x0 = torch.from_numpy(rate_util.adc_records(2, 2, 700, seed=3)).float()

    def fn(a):
        rs, pool = Resampler(500, 360, device=DEV), ResamplerPool(500, 360, leads=2, capacity=3, device=DEV)
        if a is not None:
            a.reframe(rs, "bank"), a.reframe(pool, "bank")
            _poison(pool.hist)
        out = {"records": rs.convert(fr(a, x0))}
        s0, s1 = pool.open(), pool.open()
        o = pool.push({s0: x0[0, :, :300], s1: x0[1, :, :7]})
        out["a0"], out["a1"] = o[s0], o[s1]
        o = pool.push({s0: x0[0, :, 300:301]}, close=(s1,))
        out["b0"], out["b1"] = o[s0], o[s1]
        out["c0"] = pool.close(s0, x0[0, :, 301:])
        torch.cuda.synchronize()
        return out

    got, _ = both(abi, fn)
    assert _same_bits(torch.cat([got["a0"], got["b0"], got["c0"]], dim=1), got["records"][0])


def _tight(a, lists, dtype=torch.int32):
    """per-record lists -> ((R, cap) padded with -1, (R,) counts) with cap the largest count: no spare column.  In the framed
    run the padding of the shorter rows holds the pattern instead: values beyond count are never read"""
    from ecg_denoise_amd.intake import pad_rows
    cap = max(len(r) for r in lists)
    assert cap >= 1
    pad = torch.from_numpy(pad_rows(lists, -1, shape=(len(lists), cap))).to(dtype)
    count = torch.tensor([len(r) for r in lists], dtype=torch.int32)
    if a is not None:
        pad[torch.arange(cap)[None, :] >= count[:, None]] = fu.WORD
    return fr(a, pad), fr(a, count)


@covers("ral_beat_records", "ral_beat_pool", "ral_beat_match", "ral_rhythm_records", "ral_rhythm_pool")
def test_beats_and_rhythm(abi):
    """BeatDetector, BeatPool, match_beats, BeatClassifier and BeatClassPool on beat_util's 3 x 2 x 3000 records.  The pools get
    1500 samples, then the rest at close; their histories start pattern-filled.  The classifier and the matcher take beat lists
    whose cap is the largest count.  ral_rhythm_pool's scratch is exactly ral_rhythm_pool_scratch_bytes (the wrapper adds
    nothing); new_pos is the wrapper's torch.cat, which the framed allocation frames as well."""
    from ecg_denoise_amd.beats import BeatDetector, BeatPool, match_beats
    from ecg_denoise_amd.intake import Beats
    from ecg_denoise_amd.rhythm import BeatClassifier, BeatClassPool
    x0 = _ecg(6)                                            # (3, 2, 3000), clean
    lists = BeatDetector(device=DEV).detect(x0.to(DEV)).tolist()
    shifted = [[p + 3 for p in r[1:]] for r in lists]      # a detection list to match: one miss, the rest 3 samples late

    def fn(a):
        out = {}
        x = fr(a, x0)
        det, cls = BeatDetector(device=DEV), BeatClassifier(device=DEV)
        bp, cp = BeatPool(2, 3, device=DEV), BeatClassPool(2, 3, device=DEV)
        det.det.on_device()
        if a is not None:
            a.reframe(det.det, "bank"), a.reframe(bp.det, "bank"), a.reframe(cp.beats.det, "bank")
            _poison(bp.hist), _poison(cp.beats.hist)
        b = det.detect(x)
        out["peaks"], out["count"] = b.peaks, b.count
        beats = Beats(*_tight(a, lists))
        out["match"] = match_beats(beats, Beats(*_tight(a, shifted)), device=DEV).counts
        c = cls.classify(x, beats)
        out["label"], out["corr"], out["rr"] = c.label, c.corr, c.rr_ratio
        for name, pool in (("bp", bp), ("cp", cp)):
            sids = [pool.open() for _ in range(3)]
            o1 = pool.push({s: x0[i, :, :1500] for i, s in enumerate(sids)})
            o2 = pool.push({s: x0[i, :, 1500:] for i, s in enumerate(sids[:2])}, close=sids[:2])
            o3 = pool.close(sids[2], x0[2, :, 1500:])
            for i, s in enumerate(sids):
                parts = [o1[s], o2[s] if i < 2 else o3]
                if name == "bp":
                    out[f"bp{i}"] = torch.cat([p.cpu() for p in parts])
                else:
                    for j, what in enumerate(("pos", "label", "corr", "rr")):
                        out[f"cp{i}:{what}"] = torch.cat([p[j].cpu() for p in parts])
        torch.cuda.synchronize()
        return out

    got, _ = both(abi, fn)
    pools = [args for name, args in abi.proxy.calls if name == "ral_rhythm_pool"]
    assert len(pools) == 3 and any(args[14] > 0 for args in pools)
    for args in pools:          # scratch at exactly the queried size: nothing added, nothing rounded
        want_bytes = abi.real.ral_rhythm_pool_scratch_bytes(args[14], args[8], args[9])
        assert args[16] == want_bytes and want_bytes >= 0
        if want_bytes:
            assert abi.reg.find(args[15].value).nbytes == want_bytes
    for i, r in enumerate(lists):
        assert got[f"bp{i}"].tolist() == r and got[f"cp{i}:pos"].tolist() == r
        assert _same_bits(got[f"cp{i}:label"], got["label"][i, :len(r)].cpu()) and _same_bits(got[f"cp{i}:corr"], got["corr"][i, :len(r)].cpu())
    assert got["match"][:, 0].tolist() == [len(r) - 1 for r in lists] and got["match"][:, 2].tolist() == [1, 1, 1]


@covers("ral_delineate_records", "ral_pst_records", "ral_template_records", "ral_hrv_windows", "ral_arrhythmia_windows")
def test_beat_measurements(abi):
    """BeatDelineator, PStMeasurer, MedianBeat (windows of 4 s every 2 s: three windows), HrvAnalyzer with a spectrum and
    ArrhythmiaAnalyzer with and without the P input, on beat_util's 3 x 2 x 3000 records and on two 70 s rhythms of
    synth.make_beats_with_hrv; every beat list has the largest count as its cap.  An ST level may be a NaN: the count of pattern
    words is taken on bits."""
    from ecg_denoise_amd import synth
    from ecg_denoise_amd.arrhythmia import ArrhythmiaAnalyzer
    from ecg_denoise_amd.beats import BeatDetector
    from ecg_denoise_amd.delineate import BeatDelineator
    from ecg_denoise_amd.hrv import HrvAnalyzer
    from ecg_denoise_amd.intake import Beats
    from ecg_denoise_amd.pst import PStMeasurer
    from ecg_denoise_amd.rhythm import BeatClasses, BeatClassifier
    from ecg_denoise_amd.template import MedianBeat
    x0 = _ecg(6)
    T = x0.shape[2]
    det = BeatDetector(device=DEV).detect(x0.to(DEV))
    lists = det.tolist()
    cap = max(len(r) for r in lists)
    lab0 = BeatClassifier(device=DEV).classify(x0.to(DEV), Beats(det.peaks[:, :cap].contiguous(), det.count)).label
    T2 = 360 * 70
    long_beats, long_labels = synth.make_beats_with_hrv(2, T2, seed=12, p_v=0.1)

    def fn(a):
        out = {}
        x = fr(a, x0)
        beats = Beats(*_tight(a, lists))
        f = BeatDelineator(device=DEV).delineate(x, beats)
        out.update(on=f.on, off=f.off, tpeak=f.tpeak, tend=f.tend)
        p = PStMeasurer(device=DEV).measure(x, f)
        out.update(pon=p.pon, ppeak=p.ppeak, poff=p.poff, st=p.st)
        labels = fr(a, lab0)
        t = MedianBeat(win_s=4, hop_s=2, device=DEV).average(x, beats, labels)
        out.update(tpl=t.template, used=t.used, total=t.total, rr=t.rr)
        classes = BeatClasses(labels, None, None, beats.count, beats.peaks, 0.7, 0.8)
        aa = ArrhythmiaAnalyzer(win_s=4, hop_s=2, min_m=2, device=DEV).analyse(beats, T, classes, p)
        out.update(arr_counts=aa.counts, arr_stats=aa.stats, arr_flags=aa.flags)
        lb = Beats(*_tight(a, long_beats))
        ll, _ = _tight(a, long_labels)
        lc = BeatClasses(ll, None, None, lb.count, lb.peaks, 0.7, 0.8)
        hv = HrvAnalyzer(win_s=30, hop_s=20, device=DEV)
        if a is not None:
            hv.engine.band = a.F(torch.from_numpy(hv.geometry["band"]))
        h = hv.analyse(lb, T2, lc, psd=True)
        out.update(hrv_counts=h.counts, hrv_stats=h.stats, hrv_psd=h.psd)
        a2 = ArrhythmiaAnalyzer(device=DEV).analyse(lb, T2, lc)
        out.update(arr2_counts=a2.counts, arr2_stats=a2.stats, arr2_flags=a2.flags)
        torch.cuda.synchronize()
        return out

    got, _ = both(abi, fn)
    assert got["tpl"].shape[1] == 3 and got["hrv_counts"].shape[0] == 2 * ((T2 - 30 * 360) // (20 * 360) + 1)
    assert int(got["hrv_counts"][:, 1].max()) >= 16 and torch.isfinite(got["hrv_psd"]).any(), "no window had a spectrum"
    assert int((got["on"] >= 0).sum()) > 0
