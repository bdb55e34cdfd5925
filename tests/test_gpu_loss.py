"""ral_loss_mean: F.mse_loss / SNR / RMSE (denoise_train.py:53,58-59; local_utils/evaluate.py:10-51) with the mean finished on
the device - the last workgroup to arrive scales the sum and puts the accumulator back to zero, so a training step has no
fill kernel in front of the loss and no division behind it."""
import ctypes as C

import pytest
import torch

from ecg_denoise_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# k_loss_w has 256 workgroups of 8 waves and a wave takes its windows two at a time, w and w + 2048: the second window of a pair
# exists only beyond 2048 windows.  (2049, 8): window 0 alone has a partner; (4097, 4): every window of the first pass has one
# and the last window is alone in a second pass; (6000, 8): a ragged second half; (5, 1028): n / 4 = 257, one live lane (the
# others on the clamped index) in the second pass over the window
PAIRED = [(2049, 8, 2049), (4097, 4, 4097), (6000, 8, 6000), (5, 1028, 5)]


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


@pytest.mark.parametrize("B,n,gw", [(37, 1024, 37), (2048, 512, 8192), (5, 1022, 5), (1, 4, 3)] + PAIRED)
def test_loss_mean_equals_the_host_formula_and_resets_its_scratch(B, n, gw):
    g = torch.Generator().manual_seed(B + n)
    pred = torch.randn(B, n, generator=g).to(DEV); tgt = torch.randn(B, n, generator=g).to(DEV)
    scratch = torch.zeros(2, dtype=torch.float64, device=DEV)
    L = _lib.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ref_mse = ((pred.double() - tgt.double()) ** 2).mean(1)
    for rep in range(3):                       # the scratch must come back to zero after every call
        loss = torch.full((1,), float("nan"), dtype=torch.float64, device=DEV)
        dy = torch.empty_like(pred); snr = torch.empty(B, device=DEV); rmse = torch.empty(B, device=DEV)
        _lib.check(L.ral_loss_mean(_vp(pred), _vp(tgt), n, B, gw, _vp(dy), _vp(snr), _vp(rmse), _vp(loss), _vp(scratch), s))
        torch.cuda.synchronize()
        assert abs(loss.item() - ref_mse.sum().item() / gw) <= 2e-7 * ref_mse.sum().item() / gw     # per-window sums are fp32
        assert scratch.view(torch.int64).abs().sum().item() == 0
        assert torch.allclose(dy.double(), 2.0 * (pred.double() - tgt.double()) / (gw * n), rtol=1e-6, atol=0)
        assert torch.allclose(rmse.double(), ref_mse.sqrt(), rtol=1e-6)
        ref_snr = 10 * torch.log10((tgt.double() ** 2).mean(1) / ref_mse)
        assert torch.allclose(snr.double(), ref_snr, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("B,n,gw", [(37, 1024, 37), (2048, 512, 8192), (5, 1022, 5)] + PAIRED)
def test_loss_means_carry_the_metric_means(B, n, gw):
    """ral_loss_means: the batch means of SNR and RMSE (what denoise_train.py:58-64 logs per step) leave the loss kernel
    with the loss - sums of the per-window fp32 values in double, divided by the global window count."""
    g = torch.Generator().manual_seed(3 * B + n)
    pred = torch.randn(B, n, generator=g).to(DEV); tgt = torch.randn(B, n, generator=g).to(DEV)
    scratch = torch.zeros(64, dtype=torch.float64, device=DEV)
    L = _lib.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ref_mse = ((pred.double() - tgt.double()) ** 2).mean(1)
    for rep in range(3):
        means = torch.full((3,), float("nan"), dtype=torch.float64, device=DEV)
        dy = torch.empty_like(pred); snr = torch.empty(B, device=DEV); rmse = torch.empty(B, device=DEV)
        _lib.check(L.ral_loss_means(_vp(pred), _vp(tgt), n, B, gw, _vp(dy), _vp(snr), _vp(rmse), _vp(means), _vp(scratch), s))
        torch.cuda.synchronize()
        assert abs(means[0].item() - ref_mse.sum().item() / gw) <= 2e-7 * ref_mse.sum().item() / gw
        assert abs(means[1].item() - snr.double().sum().item() / gw) <= 1e-12 * abs(snr.double().sum().item() / gw) + 1e-300
        assert abs(means[2].item() - rmse.double().sum().item() / gw) <= 1e-12 * rmse.double().sum().item() / gw
        assert scratch.view(torch.int64).abs().sum().item() == 0
        assert torch.allclose(rmse.double(), ref_mse.sqrt(), rtol=1e-6)


# ---------------------------------------------------------------------------------------------------------------------
# degenerate windows: a lead-off target is all zero, a perfect (or passed-through) prediction equals its target.  The
# reference's SNR (local_utils/evaluate.py:51), 10 log10(mean y^2 / mean (y - pred)^2), is then -inf, +inf, or NaN where both hold.
# ---------------------------------------------------------------------------------------------------------------------
DEGENERATE = {"all three": ("zero", "equal", "both"), "zero target": ("zero",), "equal": ("equal",)}


def _degenerate(B, n, kinds):
    """(pred, target, {window: kind}): randn with window 1 / B // 2 / B - 1 made degenerate ((2049, 8): window 2048 is the second
    window of k_loss_w's only pair)"""
    g = torch.Generator().manual_seed(7 * B + n)
    pred = torch.randn(B, n, generator=g); tgt = torch.randn(B, n, generator=g)
    where = dict(zip((1, B // 2, B - 1), kinds))
    for w, kind in where.items():
        if kind in ("zero", "both"):
            tgt[w] = 0.0
        if kind == "equal":
            pred[w] = tgt[w]
        if kind == "both":
            pred[w] = 0.0
    return pred.to(DEV), tgt.to(DEV), where


def _cls(v):
    v = float(v)
    return "nan" if v != v else "+inf" if v == float("inf") else "-inf" if v == float("-inf") else "finite"


def _check_degenerate(B, where, pred, tgt, dy, snr, rmse, gw, n):
    ref_mse = ((pred.double() - tgt.double()) ** 2).mean(1)
    ref_snr32 = 10 * torch.log10((tgt ** 2).mean(-1) / ((tgt - pred) ** 2).mean(-1))       # the reference formula in fp32
    ref_rmse32 = torch.sqrt(((tgt - pred) ** 2).mean(-1))
    want = {"zero": "-inf", "equal": "+inf", "both": "nan"}
    for w, kind in where.items():
        assert _cls(ref_snr32[w]) == want[kind]
        assert _cls(snr[w]) == want[kind], (w, kind, snr[w].item())
        if kind != "zero":
            assert ref_rmse32[w].item() == 0.0 and rmse[w].item() == 0.0, (w, kind, rmse[w].item())
    rest = torch.tensor([w not in where for w in range(B)], device=DEV)
    assert torch.isfinite(snr[rest]).all() and torch.isfinite(rmse).all()
    ref_snr = 10 * torch.log10((tgt.double() ** 2).mean(1) / ref_mse)
    assert torch.allclose(snr.double()[rest], ref_snr[rest], rtol=1e-5, atol=1e-5)
    assert torch.allclose(rmse.double(), ref_mse.sqrt(), rtol=1e-6)
    assert torch.allclose(dy.double(), 2.0 * (pred.double() - tgt.double()) / (gw * n), rtol=1e-6, atol=0)
    return ref_mse


@pytest.mark.parametrize("kinds", list(DEGENERATE), ids=lambda k: k.replace(" ", "-"))
@pytest.mark.parametrize("B,n", [(5, 1024), (5, 1022), (2049, 8)])
def test_loss_mean_on_degenerate_windows(B, n, kinds):
    """k_loss_w (n a multiple of 4) and k_loss (n = 1022): SNR is -inf / +inf / NaN exactly on the windows where the reference
    formula in fp32 is, RMSE is exactly 0 where the prediction equals the target, every other window keeps its tolerance, the loss
    stays finite and right, and the scratch returns to zero"""
    pred, tgt, where = _degenerate(B, n, DEGENERATE[kinds])
    gw = B
    scratch = torch.zeros(2, dtype=torch.float64, device=DEV)
    L = _lib.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for rep in range(2):
        loss = torch.full((1,), float("nan"), dtype=torch.float64, device=DEV)
        dy = torch.empty_like(pred); snr = torch.empty(B, device=DEV); rmse = torch.empty(B, device=DEV)
        _lib.check(L.ral_loss_mean(_vp(pred), _vp(tgt), n, B, gw, _vp(dy), _vp(snr), _vp(rmse), _vp(loss), _vp(scratch), s))
        torch.cuda.synchronize()
        ref_mse = _check_degenerate(B, where, pred, tgt, dy, snr, rmse, gw, n)
        assert abs(loss.item() - ref_mse.sum().item() / gw) <= 2e-7 * ref_mse.sum().item() / gw
        assert scratch.view(torch.int64).abs().sum().item() == 0


@pytest.mark.parametrize("kinds", list(DEGENERATE), ids=lambda k: k.replace(" ", "-"))
@pytest.mark.parametrize("B,n", [(5, 1024), (5, 1022), (2049, 8)])
def test_loss_means_on_degenerate_windows(B, n, kinds):
    """ral_loss_means on the same inputs: means[1] has the class (finite, +inf, -inf, NaN) of the fp64 sum of the per-window SNR
    values the call returned - NaN with all three windows, -inf with the zero target alone, +inf with the equal window alone -
    while the loss and the RMSE mean stay finite and right; the 64-double scratch returns to zero although NaN and inf passed
    through its accumulators"""
    pred, tgt, where = _degenerate(B, n, DEGENERATE[kinds])
    gw = B
    scratch = torch.zeros(64, dtype=torch.float64, device=DEV)
    L = _lib.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for rep in range(2):
        means = torch.full((3,), float("nan"), dtype=torch.float64, device=DEV)
        dy = torch.empty_like(pred); snr = torch.empty(B, device=DEV); rmse = torch.empty(B, device=DEV)
        _lib.check(L.ral_loss_means(_vp(pred), _vp(tgt), n, B, gw, _vp(dy), _vp(snr), _vp(rmse), _vp(means), _vp(scratch), s))
        torch.cuda.synchronize()
        ref_mse = _check_degenerate(B, where, pred, tgt, dy, snr, rmse, gw, n)
        assert abs(means[0].item() - ref_mse.sum().item() / gw) <= 2e-7 * ref_mse.sum().item() / gw
        assert _cls(means[1]) == _cls(snr.double().sum()) == {"all three": "nan", "zero target": "-inf", "equal": "+inf"}[kinds]
        assert abs(means[2].item() - rmse.double().sum().item() / gw) <= 1e-12 * rmse.double().sum().item() / gw
        assert scratch.view(torch.int64).abs().sum().item() == 0
