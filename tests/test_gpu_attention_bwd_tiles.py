"""The one-sweep attention backward (k_attn_bwd_mh at N >= 256, k_attn_bwd_m at N <= 128; ral_attnm.hip) tile by tile.

The operator goes through ral_attention_forward / ral_attention_backward and is compared with the fp64 autograd
restatement of tests/test_gpu_attention.py, but the error is taken PER 16-TOKEN TILE (dq per query tile, dk and dv per key
tile, per window and head): a fault confined to the last key tile of a wave, or to the tile the R-wave table window cuts,
is 1 / 16 .. 1 / 32 of a tensor norm and would pass a whole-tensor bound.  dtable is taken as a whole.

Shapes: the smallest that still reach every path of the two kernels.
  * (256, 2, 24, 3), (256, 2, 0, 2): the long-window kernel at its smallest N - one item per window, two heads of four
    waves; off = 116, so the table window starts and ends inside a tile and query tiles lie before, inside and after it
  * (512, 2, 8, 1): a table window inside one tile pair
  * (128, 2, 24, 3), (64, 2, 0, 3): one wave per head; (32, 2, 24, 3): two heads per wave, a table wider than a tile

Bound: 2e-5, the operator tolerance of tests/test_gpu_attention.py.  The build before the tile-body trim was measured on
exactly these inputs first; its worst tile is written next to each group of cases below (the rule: 2e-5 provided that
build's worst tile stays under 1e-5, otherwise twice its worst tile)."""
import ctypes as C
import functools

import pytest
import torch

from ecg_denoise_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = 16
BOUND = 2e-5


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bias_full(table, Len, N):
    H = table.shape[1]
    b = torch.zeros(H, N, N, dtype=table.dtype)
    off = (N - Len) // 2
    i = torch.arange(Len)
    idx = i[:, None] - i[None, :] + Len - 1
    b[:, off:off + Len, off:off + Len] = table[idx].permute(2, 0, 1)
    return b


@functools.lru_cache(maxsize=None)
def _reference(N, H, Len, B, seed, scales):
    """inputs (fp32, host) and the fp64 gradients; computed once per case and shared, never modified"""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, 3 * H, N, 4, generator=g)
    qkv[:, :H] *= 0.5 * scales[0]
    qkv[:, H:2 * H] *= scales[1]
    qkv[:, 2 * H:] *= scales[2]
    table = 0.5 * torch.randn(2 * Len - 1, H, generator=g) if Len else None
    do = torch.randn(B, H, N, 4, generator=g) * scales[3]
    q, k, v = (t.double().requires_grad_(True) for t in (qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]))
    tb = table.double().requires_grad_(True) if Len else None
    s = q @ k.transpose(-1, -2)
    if Len:
        s = s + _bias_full(tb, Len, N)[None]
    o_ref = torch.softmax(s, -1) @ v
    gr = torch.autograd.grad((o_ref * do.double()).sum(), [q, k, v] + ([tb] if Len else []))
    ref = {"dq": 0.5 * gr[0], "dk": gr[1], "dv": gr[2]}     # q = 0.5 (h Wq^T + b): the operator's dq carries the 0.5
    if Len:
        ref["dtable"] = gr[3]
    return qkv, table, do, ref


def _backward(N, H, Len, B, qkv, table, do, calls=1):
    """-> list of (dqkv, dtable) of `calls` backward calls on the same inputs (host tensors)"""
    qd, dod = qkv.to(DEV), do.to(DEV)
    td = table.to(DEV) if Len else None
    o = torch.empty(B, H, N, 4, device=DEV)
    lse = torch.empty(B, H, N, device=DEV)
    L = _lib.lib()
    _lib.check(L.ral_attention_forward(_vp(qd), _vp(o), _vp(lse), _vp(td), N, H, Len, B, _stream()))
    ns = L.ral_attention_backward_scratch_floats(N, H, Len, int(bool(Len)), B)
    assert ns >= 0, L.ral_last_error()
    out = []
    for _ in range(calls):
        dqkv = torch.full_like(qd, float("nan"))           # every element must be written
        gt = torch.zeros_like(td) if Len else None
        scratch = torch.empty(max(ns, 1), device=DEV)
        _lib.check(L.ral_attention_backward(_vp(qd), _vp(o), _vp(dod), _vp(lse), _vp(td), _vp(gt), _vp(dqkv), _vp(scratch),
                                            ns, N, H, Len, B, _stream()))
        torch.cuda.synchronize()
        out.append((dqkv.cpu(), gt.cpu() if Len else None))
    return out


def _tile_errors(N, H, Len, B, seed, scales=(1.0, 1.0, 1.0, 1.0)):
    """worst relative L2 over the (window, head, 16-token tile) blocks of dq, dk, dv; dtable as a whole.  NaN stays NaN."""
    qkv, table, do, ref = _reference(N, H, Len, B, seed, tuple(scales))
    dqkv, gt = _backward(N, H, Len, B, qkv, table, do)[0]
    errs = {}
    for name, got in (("dq", dqkv[:, :H]), ("dk", dqkv[:, H:2 * H]), ("dv", dqkv[:, 2 * H:])):
        r = ref[name].reshape(B, H, N // TILE, TILE * 4)
        d = got.double().reshape(B, H, N // TILE, TILE * 4) - r
        rel = d.norm(dim=-1) / r.norm(dim=-1)
        errs[name] = float("nan") if torch.isnan(rel).any() else rel.max().item()
    if Len:
        errs["dtable"] = ((gt.double() - ref["dtable"]).norm() / ref["dtable"].norm()).item()
    return errs


def _check(errs, what):
    print(what, {k: f"{v:.3e}" for k, v in errs.items()})       # (the figures, before the assertion)
    assert all(e == e and e < BOUND for e in errs.values()), (what, errs)


# Worst tile of the build before the trim on these inputs: 1.21e-6 (dk of (512, 2, 8, 1)); dq 1.05e-6, dv 1.09e-6,
# dtable 3.3e-7 - more than a factor 2 under 1e-5, so the bound is the operator tolerance.
@pytest.mark.parametrize("N,H,Len,B", [
    (256, 2, 24, 3), (256, 2, 0, 2), (512, 2, 8, 1),      # k_attn_bwd_mh
    (128, 2, 24, 3), (64, 2, 0, 3), (32, 2, 24, 3),       # k_attn_bwd_m
])
def test_backward_tiles_against_fp64(N, H, Len, B):
    _check(_tile_errors(N, H, Len, B, seed=N + Len), (N, H, Len, B))


# Worst tile of the build before the trim on these inputs: 1.62e-6 (dq of (128, 2, 24) with v at 1e6); dk 1.32e-6,
# dv 1.08e-6, dtable 8.5e-7.
@pytest.mark.parametrize("N,H,Len", [(256, 2, 24), (128, 2, 24)])
@pytest.mark.parametrize("scales", [
    (1e-3, 1e-3, 1.0, 1.0), (1e4, 1e-4, 1.0, 1.0),        # the sets that take the independent-scale path of q and k
    (1.0, 1.0, 1.0, 1e-12), (1.0, 1.0, 1.0, 1e8),         # dO and v: the operands of the first piece of dS
    (1.0, 1.0, 1e-6, 1.0), (1.0, 1.0, 1e6, 1.0),
])
def test_backward_tiles_operand_ranges(N, H, Len, scales):
    """The shapes tests/test_gpu_attention.py::test_attention_operator_operand_ranges leaves out, per tile."""
    _check(_tile_errors(N, H, Len, 3, seed=11, scales=scales), (N, H, Len, scales))


@pytest.mark.parametrize("N,H,Len,B", [(256, 2, 24, 3), (128, 2, 24, 3), (32, 2, 24, 3), (64, 2, 0, 3)])
def test_backward_is_deterministic(N, H, Len, B):
    """Two calls on the same inputs: dq, dk, dv bit for bit - and dtable, which the build before the trim also repeated
    bit for bit on these inputs (its LDS sums are doubles, rounded to fp32 once per workgroup)."""
    qkv, table, do, _ = _reference(N, H, Len, B, N + Len, (1.0, 1.0, 1.0, 1.0))
    (a, ta), (b, tb) = _backward(N, H, Len, B, qkv, table, do, calls=2)
    assert not torch.isnan(a).any()
    assert torch.equal(a[:, :H], b[:, :H]), "dq"
    assert torch.equal(a[:, H:2 * H], b[:, H:2 * H]), "dk"
    assert torch.equal(a[:, 2 * H:], b[:, 2 * H:]), "dv"
    if Len:
        assert torch.equal(ta, tb), "dtable"
