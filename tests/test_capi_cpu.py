"""CPU-side checks of the C ABI: the library loads, exports every symbol that
include/ralenet.h declares, and its host-only entry points (layout, PE tables, config
validation) agree with the reference contract.  No compute calls (no GPU here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ralenet_oracle as O
from ecg_denoise_amd import _lib
from ecg_denoise_amd.model import pe_table_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_header_symbols():
    hdr = open(os.path.join(ROOT, "include", "ralenet.h")).read()
    declared = set(re.findall(r"\b(ral_[a-z_0-9]+)\s*\(", hdr))
    declared -= {"ral_handle"}
    L = C.CDLL(_lib.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(L, name), f"{name} declared in ralenet.h but not exported"
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)


@pytest.mark.parametrize("variant", ["nra", "full", "mlp"])
@pytest.mark.parametrize("leads", [1, 2])
def test_layout_matches_reference_state_dict(variant, leads, golden_dir):
    cfg = _lib.make_config(variant, leads, 512, 4, 1)
    ent = _lib.layout(cfg)
    shapes = O.ralenet_param_shapes(variant, leads)
    mine = [(e["name"], tuple(e["shape"])) for e in ent if e["kind"] == _lib.KIND_PARAM]
    assert mine == [(k, tuple(s)) for k, s in shapes.items()]
    # golden key list comes from the reference's own named_parameters()
    if leads == 2:
        g = np.load(os.path.join(golden_dir, f"g3_{variant}_l2_L256.npz"))
        assert [str(k) for k in g["keys"]] == [n for n, _ in mine]
    segs = sorted((e["offset"], e["offset"] + int(np.prod(e["shape"]))) for e in ent if e["kind"] == _lib.KIND_PARAM)
    assert all(a[1] <= b[0] for a, b in zip(segs, segs[1:]))
    assert all(s[0] % 4 == 0 for s in segs)  # 16-byte aligned tensors
    assert segs[-1][1] <= _lib.lib().ral_param_floats(C.byref(cfg))
    names = [e["name"] for e in ent]
    assert "conv1.2.running_mean" in names and "conv1.2.num_batches_tracked" in names
    n_expected = {"nra": 303, "full": 311, "mlp": 293}[variant]  # reference state_dict sizes
    assert len(ent) == n_expected
    total = sum(int(np.prod(s)) for _, s in mine)
    if leads == 2:
        assert total == {"nra": 1086800, "full": 1087282, "mlp": 1087228}[variant]


def test_danet_layout_matches_reference_state_dict(golden_dir):
    """every state_dict entry of the reference's Seq2Seq2, in its order (the fixture's gradient keys are the reference's
    named_parameters(), its after_* keys the buffers); fcn2.* alias fcn1.*; bad configurations are rejected"""
    import danet_oracle as D
    cfg = _lib.make_config("danet", 2, 512, 4, 1)
    ent = _lib.layout(cfg)
    shapes = D.danet_state_shapes()
    assert [(e["name"], tuple(e["shape"])) for e in ent] == [(k, tuple(s)) for k, s in shapes.items()]
    g = np.load(os.path.join(golden_dir, "g3_danet_L512.npz"))
    ref_params = [k[5:] for k in g.files if k.startswith("grad_")]
    assert ref_params == [e["name"] for e in ent if e["kind"] == _lib.KIND_PARAM and ".dam.fcn2." not in e["name"]]
    assert sorted(k[6:] for k in g.files if k.startswith("after_")) == sorted(e["name"] for e in ent if e["kind"] != _lib.KIND_PARAM)
    off = {e["name"]: (e["kind"], e["offset"]) for e in ent}
    for k in off:
        if ".dam.fcn2." in k:
            assert off[k] == off[k.replace(".dam.fcn2.", ".dam.fcn1.")]
    assert sum(int(np.prod(e["shape"])) for e in ent if e["kind"] == _lib.KIND_PARAM and ".dam.fcn2." not in e["name"]) == 18009
    for leads, L in ((1, 512), (2, 520), (2, 16)):
        bad = _lib.make_config("danet", leads, L, 4, 1)
        assert _lib.lib().ral_layout_count(C.byref(bad)) == -1


def test_pe_table_matches_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "pe_tables.npz"))
    for lvl, Cc in enumerate(O.CHANNELS):
        p = pe_table_host(1024, lvl)
        ref = O.pe_table(1024 >> lvl, Cc).numpy()
        n = min(64, p.shape[0])
        assert np.abs(p[:n] - g[f"C{Cc}"][:n]).max() < 5e-7
        # libm vs torch differ by an ulp in pow/sin arguments: bounded by ulp(pos) ~ 6e-5 at pos~1000
        assert np.abs(p - ref).max() < 2e-4


@pytest.mark.parametrize("kw,msg", [
    (dict(L=500), "multiple of 16"), (dict(L=2048), "multiple of 16"), (dict(L=16), "at least 32"), (dict(leads=3), "leads"),
    (dict(max_batch=0), "max_batch"),
])
def test_config_validation(kw, msg):
    args = dict(variant="full", leads=2, L=512, max_batch=4, train=1)
    args.update(kw)
    cfg = _lib.make_config(**args)
    assert _lib.lib().ral_param_floats(C.byref(cfg)) < 0
    assert msg in _lib.lib().ral_last_error().decode()


def test_workspace_scales_with_batch():
    a = _lib.lib().ral_workspace_bytes(C.byref(_lib.make_config("full", 2, 512, 32, 1)))
    b = _lib.lib().ral_workspace_bytes(C.byref(_lib.make_config("full", 2, 512, 64, 1)))
    c = _lib.lib().ral_workspace_bytes(C.byref(_lib.make_config("full", 2, 512, 64, 0)))
    assert 1.9 < b / a < 2.1 and c < b / 3


def test_product_path_has_no_cpu_fallback():
    import torch
    from ecg_denoise_amd import RALENet, RalError
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises((RalError, RuntimeError, AssertionError)):
        RALENet("full", device="cpu")
    # and the package never imports the oracle
    import ecg_denoise_amd
    pkg = os.path.dirname(ecg_denoise_amd.__file__)
    for f in os.listdir(pkg):
        if f.endswith(".py"):
            assert "oracle" not in open(os.path.join(pkg, f)).read().replace("no CPU fallback", ""), f


def test_global_option_validates_key_and_value_and_refuses_retired_switches():
    """`ral_global_option` is the only way to change a library switch (no environment variable does): unknown names - retired
    switches among them - and negative values are rejected with a message, known names are case-insensitive and accept an
    optional RAL_ prefix"""
    L = _lib.lib()
    assert L.ral_global_option(b"attn_f16", 1) == 0
    assert L.ral_global_option(b"RAL_ATTN_F16", 1) == 0
    assert L.ral_global_option(b"Unet_Eval_Grid", 512) == 0
    assert L.ral_global_option(b"no_such_switch", 1) != 0 and b"unknown switch" in L.ral_last_error()
    assert L.ral_global_option(b"mlp_hthreads", 256) != 0 and b"unknown switch" in L.ral_last_error()   # retired: a constant now
    assert L.ral_global_option(b"attn_f16", -1) != 0 and b"negative" in L.ral_last_error()
    assert L.ral_global_option(None, 1) != 0
    # grid / set counts: 0 would be a launch without a workgroup
    for k in (b"unet_eval_grid", b"dw_sets"):
        assert L.ral_global_option(k, 0) != 0 and b"out of range" in L.ral_last_error(), k
    # the others take 0 (attn_fwd_h = 0: never); a refusal here can only be the latch, which is checked after the range
    first = L.ral_global_option(b"attn_fwd_h", 0)
    assert first == 0 or b"already read" in L.ral_last_error()
    if first == 0:
        assert L.ral_global_option(b"attn_fwd_h", 256) == 0   # (back to the default before anything reads it)


def test_global_option_after_the_first_read_is_refused_not_ignored():
    """switches are latched at first use: once the library has read one, a different value is an error (the same value
    again is accepted)"""
    L = _lib.lib()
    cfg = _lib.make_config("full", 2, 512, 8, 1)
    first = L.ral_global_option(b"dw_sets", 6)                 # (an earlier test of this process may have sized a workspace)
    assert first == 0 or b"already read" in L.ral_last_error()
    assert L.ral_workspace_bytes(C.byref(cfg)) > 0             # plan_workspace reads DW_SETS
    if first == 0:
        assert L.ral_global_option(b"dw_sets", 6) == 0
    assert L.ral_global_option(b"dw_sets", 4) != 0 and b"already read" in L.ral_last_error()


def test_global_option_accepts_the_default_after_the_first_read():
    """a switch the library has read without it ever being set latches its default: setting that same value is accepted,
    any other is refused (a fresh process, so that nothing has set DW_SETS before)"""
    import subprocess
    import sys
    code = ("import ctypes as C, sys\n"
            "from ecg_denoise_amd import _lib\n"
            "L = _lib.lib()\n"
            "assert L.ral_workspace_bytes(C.byref(_lib.make_config('full', 2, 512, 8, 1))) > 0   # reads DW_SETS: 6\n"
            "assert L.ral_global_option(b'dw_sets', 6) == 0, L.ral_last_error()\n"
            "assert L.ral_global_option(b'dw_sets', 4) != 0 and b'already read' in L.ral_last_error()\n")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]


def test_library_reads_only_the_two_documented_environment_variables():
    """the product build of the library has exactly two getenv call sites outside `#ifdef RAL_DIAG`: ral_env_int (RAL_LANES,
    RAL_NO_SIDE_STREAM) - and no other source file calls getenv at all"""
    import glob
    n_outside, in_diag = 0, False
    for f in sorted(glob.glob(os.path.join(ROOT, "ecg_denoise_amd", "csrc", "*.h*"))):
        depth_diag = None
        for line in open(f):
            s = line.strip()
            if s.startswith("#ifdef RAL_DIAG"):
                in_diag = True
            elif s.startswith("#endif") and in_diag:
                in_diag = False
            elif "getenv(" in line and not s.startswith("//") and not in_diag:
                n_outside += 1
                assert f.endswith("ral_api.hip"), (f, line)
    assert n_outside == 1                      # the one inside ral_env_int
    src = "".join(open(f).read() for f in sorted(glob.glob(os.path.join(ROOT, "ecg_denoise_amd", "csrc", "*.h*"))))   # (the two callers are RA-LENet's: ral_ralenet.hip)
    assert sorted(set(re.findall(r'ral_env_int\("(RAL_[A-Z_]+)"', src))) == ["RAL_LANES", "RAL_NO_SIDE_STREAM"]


@pytest.mark.parametrize("variant,leads", [("unet", 2), ("unet", 1), ("acdae", 2)])
def test_baseline_layout_matches_reference_state_dict(variant, leads, golden_dir):
    """U-Net and ACDAE: parameter names in the reference's named_parameters() order (the fixtures' key lists), the oracle's
    shapes, tensors that do not overlap, start on 16 bytes and end inside ral_param_floats; U-Net's BatchNorm buffers follow
    their layer and tile the state buffer"""
    cfg = _lib.make_config(variant, leads, 512, 4, 1)
    ent = _lib.layout(cfg)
    shapes = O.unet_param_shapes(leads) if variant == "unet" else O.acdae_param_shapes()
    mine = [(e["name"], tuple(e["shape"])) for e in ent if e["kind"] == _lib.KIND_PARAM]
    assert mine == [(k, tuple(s)) for k, s in shapes.items()]
    if leads == 2:
        g = np.load(os.path.join(golden_dir, f"g3_{variant}_l2_L512.npz"))
        assert [str(k) for k in g["keys"]] == [n for n, _ in mine]
    segs = sorted((e["offset"], e["offset"] + int(np.prod(e["shape"]))) for e in ent if e["kind"] == _lib.KIND_PARAM)
    assert segs[0][0] == 0 and all(a[1] <= b[0] for a, b in zip(segs, segs[1:]))
    assert all(s[0] % 4 == 0 for s in segs)
    nparam = _lib.lib().ral_param_floats(C.byref(cfg))
    assert segs[-1][1] <= nparam < segs[-1][1] + 4          # (nothing after the last tensor but its padding)
    state = sorted((e["offset"], e["offset"] + int(np.prod(e["shape"]))) for e in ent if e["kind"] == _lib.KIND_STATE)
    nstate = _lib.lib().ral_state_floats(C.byref(cfg))
    if variant == "acdae":
        assert len(ent) == len(mine) == 20 and nstate == 0
    else:
        names = [e["name"] for e in ent]
        for i, n in enumerate(names):
            if n.endswith(".running_mean"):
                pre = n[:-len("running_mean")]
                assert names[i - 2:i + 3] == [pre + s for s in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
        assert len(ent) == 42 + 3 * 10 and len(state) == 20
        assert state[0][0] == 0 and all(a[1] == b[0] for a, b in zip(state, state[1:])) and state[-1][1] == nstate


def _entry(cfg, idx, cap):
    name = C.create_string_buffer(256)
    kind, ndim, off, shape = C.c_int32(), C.c_int32(), C.c_int64(), (C.c_int64 * 4)()
    rc = _lib.lib().ral_layout_entry(C.byref(cfg), idx, name, cap, C.byref(kind), C.byref(off), C.byref(ndim), shape)
    return rc, _lib.lib().ral_last_error().decode()


ALL_NETWORKS = [("nra", 1, 64), ("full", 2, 512), ("mlp", 2, 512), ("unet", 1, 16), ("acdae", 2, 64), ("danet", 2, 32)]


@pytest.mark.parametrize("variant,leads,L", ALL_NETWORKS)
def test_layout_entry_failures_say_which_argument(variant, leads, L):
    """a bad index and a short name buffer are told apart, in the same words, for every network (return code -1 as ever)"""
    cfg = _lib.make_config(variant, leads, L, 2, 1)
    n = _lib.lib().ral_layout_count(C.byref(cfg))
    assert n > 0
    _lib.lib().ral_param_floats(C.byref(_lib.make_config(variant, leads, L, 0, 1)))     # leaves another message behind
    assert _entry(cfg, -1, 256) == (-1, "entry -1 out of range")
    assert _entry(cfg, n, 256) == (-1, f"entry {n} out of range")
    assert _entry(cfg, 0, 1) == (-1, "name buffer too small")
    assert _entry(cfg, n - 1, 256)[0] == 0


@pytest.mark.parametrize("variant,leads,L", ALL_NETWORKS)
def test_pe_table_only_for_ralenet_variants(variant, leads, L):
    """the positional-encoding table is RA-LENet's: every other network is refused, at every level"""
    cfg = _lib.make_config(variant, leads, L, 2, 1)
    buf = np.full(L * 128, np.nan, np.float32)
    for level in range(-1, 6):
        rc = _lib.lib().ral_pe_table(C.byref(cfg), level, buf.ctypes.data_as(C.c_void_p), C.c_int64(buf.size))
        if variant in ("nra", "full", "mlp") and 0 <= level <= 4:
            assert rc == 0
        else:
            assert rc == -1 and _lib.lib().ral_last_error().decode() == "no PE table for this variant/level"
    if variant not in ("nra", "full", "mlp"):
        assert np.isnan(buf).all()                # (nothing was written)


_CONV13_FWD = ("x", "w", "b", "y")
_CONV13_BWD = ("x", "y", "dy", "w", "gw", "gb", "dx")
# (entry point, {argument: value} over the legal call B=2, 12 -> 6 channels, L=256, what the message must name)
_CONV13_REFUSALS = (
    [(fn, {p: None}, f"{p} is NULL") for fn, ps in (("forward", _CONV13_FWD), ("backward", _CONV13_BWD[:-1])) for p in ps]
    + [(fn, kw, msg) for fn in ("forward", "backward") for kw, msg in [
        (dict(B=0), "B must be at least 1"), (dict(B=-3), "B must be at least 1"),
        (dict(L=0), "L must be at least 1"), (dict(L=-1), "L must be at least 1"),
        (dict(cin=12, cout=12), "unsupported channel counts"), (dict(cin=13, cout=1), "unsupported channel counts"),
        (dict(cin=1, cout=13), "unsupported channel counts"), (dict(cin=0, cout=6), "unsupported channel counts"),
        (dict(L=2 ** 31 - 1), "L needs more than the 160 KB of LDS")]]
    # 12 -> 6 channels: forward rows of 12, backward rows of 18 floats per sample; the first L past 160 KB of LDS each
    + [("forward", dict(L=3324), "L needs more than the 160 KB of LDS"), ("backward", dict(L=2212), "L needs more than the 160 KB of LDS")])


@pytest.mark.parametrize("fn,kw,msg", _CONV13_REFUSALS, ids=[f"{fn}-{'-'.join(f'{k}={v}' for k, v in kw.items())}" for fn, kw, _ in _CONV13_REFUSALS])
def test_conv13_entry_points_refuse_bad_arguments_before_any_launch(fn, kw, msg):
    """ral_conv13_forward / _backward refuse a null operand (dx alone is optional), B < 1, L < 1, channel counts the kernels
    do not take and a row length whose LDS need passes the 160 KB of a CU - each with a message that names the argument, and
    before any HIP call: this runs without a device (the operand pointers are host memory that a launch would fault on)."""
    host = np.zeros(16, np.float32)
    a = dict(B=2, cin=12, cout=6, L=256)
    ptr = {p: host.ctypes.data_as(C.c_void_p) for p in _CONV13_FWD + _CONV13_BWD}
    for k, v in kw.items():
        if k in ptr:
            ptr[k] = C.c_void_p(0)
        else:
            a[k] = v
    L = _lib.lib()
    L.ral_param_floats(C.byref(_lib.make_config("full", 2, 512, 0, 1)))     # leaves another message behind
    if fn == "forward":
        rc = L.ral_conv13_forward(*(ptr[p] for p in _CONV13_FWD), a["B"], a["cin"], a["cout"], a["L"], 1, C.c_void_p(0))
    else:
        rc = L.ral_conv13_backward(*(ptr[p] for p in _CONV13_BWD), a["B"], a["cin"], a["cout"], a["L"], 1, C.c_void_p(0))
    err = L.ral_last_error().decode()
    assert rc != 0 and err.startswith(f"ral_conv13_{fn}: {msg}"), (rc, err)


def test_backward_halves_refusal_names_no_network():
    """ral_backward_begin / _end are RA-LENet's; their refusal on another handle says so without naming a network the handle
    is not (the text the GPU test of the handles asserts on real handles: no handle can be created here)"""
    src = open(os.path.join(ROOT, "ecg_denoise_amd", "csrc", "ral_api.hip")).read()
    for fn in ("ral_backward_begin", "ral_backward_end"):
        body = src[src.index(f"int {fn}(ral_handle* h"):]
        body = body[:body.index("\n}\n")]
        msgs = re.findall(r'"([^"]+)"', body)
        assert msgs == ["null handle", f"{fn}: RA-LENet handles only (the other networks: ral_backward)"], msgs
        assert not re.search(r"U-Net|ACDAE|DANet", body)
