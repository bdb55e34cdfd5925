"""The attention forward with 32x32 score blocks (k_attn_fwd_t32, ral_fwd.hip: one v_mfma_f32_32x32x16_f16 per 32 keys x
32 queries) through ral_attention_forward against an fp64 torch restatement of `softmax(q k^T + R-wave bias) v`, at the
tolerance of the operator tests of test_gpu_attention.py (relative L2 2e-5 on o and lse).

The launcher gives the kernel every window length N >= ATTN_FWD_T32 with N % 64 == 0 (default 256: the two long levels
of a 512-sample window).  `test_every_value_of_the_switch` re-runs this file in fresh processes with the switch at 0 (the
kernels the levels had before) and at 64 (the new kernel at N = 128 and 64 too, which the default leaves on the scalar
path); a case at N < 256 runs the new kernel only there."""
import ctypes as C

import pytest
import torch

from ecg_denoise_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-5
MODEL_CASE = ("full", 1, 512, 4)          # (variant, leads, L, B) of the whole-model train step


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bias_full(table, Len, N):
    H = table.shape[1]
    b = torch.zeros(H, N, N, dtype=table.dtype, device=table.device)
    off = (N - Len) // 2
    i = torch.arange(Len, device=table.device)
    idx = i[:, None] - i[None, :] + Len - 1
    b[:, off:off + Len, off:off + Len] = table[idx].permute(2, 0, 1)
    return b


def _ref(qkv, table, Len, ref_dev="cpu", chunk=256):
    """fp64 o, lse of qkv (B, 3H, N, 4; q already scaled) - on the CPU, or for the large batch in chunks on the device"""
    H = qkv.shape[1] // 3
    N = qkv.shape[2]
    bias = _bias_full(table.double().to(ref_dev), Len, N)[None] if Len else None
    o, lse = [], []
    for b0 in range(0, qkv.shape[0], chunk):
        x = qkv[b0:b0 + chunk].double().to(ref_dev)
        s = x[:, :H] @ x[:, H:2 * H].transpose(-1, -2)
        if Len:
            s = s + bias
        o.append((torch.softmax(s, -1) @ x[:, 2 * H:]).cpu())
        lse.append(torch.logsumexp(s, -1).cpu())
    return torch.cat(o), torch.cat(lse)


def _forward(qkv, table, Len, with_lse=True):
    B, H3, N, _ = qkv.shape
    H = H3 // 3
    qd = qkv.to(DEV)
    td = table.to(DEV) if Len else None
    o = torch.full((B, H, N, 4), float("nan"), device=DEV)             # every element must be written
    lse = torch.full((B, H, N), float("nan"), device=DEV) if with_lse else None
    _lib.check(_lib.lib().ral_attention_forward(_vp(qd), _vp(o), _vp(lse), _vp(td), N, H, Len, B, _stream()))
    torch.cuda.synchronize()
    return o.cpu().double(), (lse.cpu().double() if with_lse else None)


def _rel(a, b):
    return ((a - b).norm() / b.norm()).item()


def _inputs(N, H, Len, B, seed, scales=(1.0, 1.0, 1.0)):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, 3 * H, N, 4, generator=g)
    qkv[:, :H] *= 0.5 * scales[0]
    qkv[:, H:2 * H] *= scales[1]
    qkv[:, 2 * H:] *= scales[2]
    table = 0.5 * torch.randn(2 * Len - 1, H, generator=g) if Len else None
    return qkv, table


def _errs(N, H, Len, B, seed, scales=(1.0, 1.0, 1.0), ref_dev="cpu"):
    qkv, table = _inputs(N, H, Len, B, seed, scales)
    o_ref, lse_ref = _ref(qkv, table, Len, ref_dev)
    o, lse = _forward(qkv, table, Len)
    errs = {"o": _rel(o, o_ref), "lse": _rel(lse, lse_ref)}
    print(N, H, Len, B, scales, errs)
    return errs


@pytest.mark.parametrize("N,H,Len,B", [
    (512, 2, 32, 3), (512, 2, 0, 5), (256, 4, 16, 5), (256, 4, 0, 3),      # the long levels of a 512-sample window
    (128, 8, 8, 3), (128, 8, 0, 5), (64, 16, 4, 5), (64, 16, 0, 3),        # the shorter levels (new kernel with the switch at 64)
    (256, 4, 32, 3), (64, 2, 32, 3), (512, 2, 64, 2),                      # a table as wide as a block, as a query pair, as two blocks
    (256, 4, 18, 3), (192, 4, 30, 3),                                      # a table that straddles block edges; N = 3 x 64
    (1024, 2, 64, 1),                                                      # the top level of a 1024-sample window
])
def test_t32_forward_against_fp64(N, H, Len, B):
    errs = _errs(N, H, Len, B, seed=N + Len)
    assert all(e == e and e < TOL for e in errs.values()), errs            # NaN = an element left unwritten


def test_t32_forward_many_windows():
    """B = 700, and B = 2100 at N = 256 (4200 items for the 4096 persistent workgroups: some take two)"""
    for N, H, Len, B in ((512, 2, 32, 700), (256, 4, 16, 2100)):
        errs = _errs(N, H, Len, B, seed=7, ref_dev=DEV)
        assert all(e == e and e < TOL for e in errs.values()), (B, errs)


def test_t32_forward_eval_writes_no_lse():
    """lse == nullptr (the eval forward): the same o"""
    qkv, table = _inputs(512, 2, 32, 3, seed=3)
    o_ref, _ = _ref(qkv, table, 32)
    o, _ = _forward(qkv, table, 32, with_lse=False)
    assert _rel(o, o_ref) < TOL


@pytest.mark.parametrize("scales", [
    (1e4, 1e-4, 1.0, 1.0), (1e-4, 1e4, 1.0, 1.0),      # q and k twenty-six binades apart (scores still O(1))
    (1e-3, 1e-3, 1.0, 1.0),                            # scores ~1e-6: a uniform softmax
    (1.0, 1.0, 1e-6, 1.0), (1.0, 1.0, 1e6, 1.0),       # v far below / above fp16's range
    (1.0, 1.0, 1.0, 1e-12), (1.0, 1.0, 1.0, 1e8),      # (dO scales of the operator test: the forward sees the other three)
    (30.0, 1.0, 3e-5, 1e-9),
])
def test_t32_forward_operand_ranges(scales):
    """the eight scale tuples of test_attention_operator_operand_ranges at (512, 2, 32): q and k reach the f16 matrix cores
    as fp16 pairs balanced per head by a power of two, so magnitudes far outside fp16's range keep the fp32 tolerance"""
    errs = _errs(512, 2, 32, 3, seed=11, scales=scales[:3])
    assert all(e == e and e < TOL for e in errs.values()), (scales, errs)


@pytest.mark.parametrize("N,H,Len", [(512, 2, 32), (256, 4, 0), (128, 8, 8), (64, 16, 0)])
def test_t32_forward_exact_fallback(N, H, Len):
    """One query row scaled by 1e4 against an (almost) opposite key row scaled by 1e4 (as
    test_gpu_configs.py::test_attention_forward_exact_fallback): the Cauchy-Schwarz shift overshoots the row maximum by
    ~1e8 in log2 units, every term of the row underflows and the task is redone with the running-max recurrence.  The
    other rows of the task go through the redo too; untouched tasks must stay right."""
    g = torch.Generator().manual_seed(N + H)
    B = 3
    q = (torch.randn(B, H, N, 4, generator=g, dtype=torch.float64) * 0.5).float().double()
    k = torch.randn(B, H, N, 4, generator=g, dtype=torch.float64).float().double()
    v = torch.randn(B, H, N, 4, generator=g, dtype=torch.float64).float().double()
    table = (0.5 * torch.randn(2 * Len - 1, H, generator=g, dtype=torch.float64)).float() if Len else None
    rows = [(0, 0, 5, N - 3), (1, H - 1, N // 2, 1), (2, H // 2, N - 1, N // 2)]
    for (b, h, qi, ki) in rows:
        q[b, h, qi] *= 1e4
        k[b, h, ki] = -q[b, h, qi] / q[b, h, qi].norm() * k[b, h, ki].norm() * 1e4    # q.k = -|q||k|: bound maximally loose
    qkv = torch.cat([q, k, v], 1).float()
    o_ref, lse_ref = _ref(qkv, table, Len)
    o, lse = _forward(qkv, table, Len)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    print(N, H, Len, "o", _rel(o, o_ref))
    assert _rel(o, o_ref) < 1e-5
    for (b, h, qi, ki) in rows:        # the redone rows themselves (scores ~1e4: fp32 products carry ~1e-3 absolute error)
        assert _rel(o[b, h, qi], o_ref[b, h, qi]) < 2e-2, (b, h, qi)
    # scores of magnitude |q| |k| ~ 1e4 reach every row of the scaled key's head: their fp32 rounding, ~|q| |k| 2^-23, is
    # what a nearly cancelling score leaves in any summation order, so lse is compared to that bound
    qf, kf = qkv[:, :H].double(), qkv[:, H:2 * H].double()
    scale = (qf.norm(dim=-1) * kf.norm(dim=-1).amax(-1, keepdim=True)).clamp_min(1.0)
    assert ((lse - lse_ref).abs() / scale).max().item() < 1e-6


def test_t32_forward_keeps_non_finite_values_in_their_head():
    """no clamp: a NaN in q and an Inf in k reach the outputs of their own head and no other"""
    for N, H, Len in ((512, 2, 32), (256, 4, 16)):
        qkv, table = _inputs(N, H, Len, 2, seed=5)
        qkv[1, 0, 5, 2] = float("nan")                 # q of head 0, window 1
        qkv[0, H + 1, 70, 1] = float("inf")            # k of head 1, window 0
        o, lse = _forward(qkv, table, Len)
        assert not torch.isfinite(o[1, 0, 5]).all() and not torch.isfinite(lse[1, 0, 5])
        assert not torch.isfinite(o[0, 1]).all()
        keep = torch.ones(2, H, dtype=torch.bool)
        keep[1, 0] = keep[0, 1] = False
        assert torch.isfinite(o[keep]).all() and torch.isfinite(lse[keep]).all()
        o_ref, _ = _ref(qkv, table, Len)
        assert _rel(o[keep], o_ref[keep]) < TOL


def test_t32_whole_model_train_step_matches_oracle():
    """forward + backward of RA-LENet "full" at 4 x 1 x 512 against the fp64 oracle, at the per-tensor parity bars of
    test_gpu_parity.py (the backward reads the o and lse this forward wrote)"""
    from parity_bars import bars, check
    from parity_util import parity_yardstick, run_parity
    res, _, _ = run_parity(*MODEL_CASE, DEV, trace=False)
    yard = parity_yardstick(*MODEL_CASE, trace=False)
    check(res, bars(yard), yard, what="t32 %s leads=%d L=%d B=%d" % MODEL_CASE)


@pytest.mark.parametrize("opts", ["attn_fwd_t32=0", "attn_fwd_t32=64"])
def test_every_value_of_the_switch(opts):
    """The switch is read once per process: 0 (never: every level on the kernel it had before) and 64 (the new kernel at
    N = 128 and 64 too) run the comparisons of this file in a process of their own (tests/conftest.py applies RAL_TEST_OPTIONS)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-k", "not every_value_of_the_switch"],
                       env=dict(os.environ, RAL_TEST_OPTIONS=opts), cwd=root, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
