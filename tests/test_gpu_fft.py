"""FFT-threshold baseline on the GPU (ral_fft_denoise through `ecg_denoise_amd.fft_denoise`) against the fp64 restatement of
local_utils/denoisefunc.py:36-66 (tests/fft_util.py).  Kept-bin counts must be equal; outputs within 1e-5 relative L2 per group,
the project's fp32 tolerance for the wavelet baseline (tests/test_gpu_baselines.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import fft_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5

FFT_L = (16, 18, 20, 30, 256, 360, 1000, 1024, 7680, 8192)
DIRECT_L = (2, 17, 112, 375, 1008, 1022)
AMPS12 = (1.0, 0.3, 0.02, 0.6, 0.1, 0.02, 0.8, 0.05, 0.3, 0.02, 0.5, 0.2)
SHAPES = {"1x1": (1, (1.0,)), "3x2": (3, (1.0, 0.3)), "2x3": (2, (1.0, 0.3, 0.02)), "2x12": (2, AMPS12), "5": (5, (1.0,))}
CASES = [(L, s) for L in FFT_L + DIRECT_L for s in ("1x1", "3x2", "2x3", "5")] + [(1024, "2x12"), (8192, "2x12")]


def _check(x, y, kept, threshold=U.THRESHOLD, min_margin=1e-2, what=""):
    """both checks of a result against the restatement -> the groups that were compared"""
    ref, rkept, margin = U.fft_denoise_ref(x, threshold)
    ok = margin >= min_margin
    err = U.rel_l2(y, ref)
    print(what, "groups", len(ref), "compared", int(ok.sum()), "min margin %.3g" % margin.min(), "worst rel-L2 %.3g" % err[ok].max(),
          "kept equal", bool(np.array_equal(np.asarray(kept)[ok], rkept[ok])))
    assert np.array_equal(np.asarray(kept)[ok], rkept[ok]), (what, np.asarray(kept)[ok], rkept[ok])
    assert err[ok].max() < TOL, (what, err)
    return ok


@pytest.mark.parametrize("L,shape", CASES)
def test_designed_inputs_match_the_restatement(L, shape):
    from ecg_denoise_amd import fft_denoise
    groups, amps = SHAPES[shape]
    x = U.designed(groups, amps, L, seed=7 * L + len(amps))
    if shape == "5":
        x = x.reshape(5, L)                                 # 2-D: every row against its own maximum
    y, kept = fft_denoise(x, return_kept=True)
    assert y.shape == x.shape and y.dtype == np.float32 and kept.shape == (groups,) and kept.dtype == np.int32
    assert _check(x, y, kept, what=f"L={L} {shape}").all()
    for l, amp in enumerate(amps):                          # a lead of amplitude 0.02 is below the group's cutoff everywhere:
        if amp < 1.25 * U.THRESHOLD and len(amps) > 1:      # exactly zero under the group rule, not under a per-row rule
            assert not np.any(y[:, l]), (L, shape, l)
            assert np.all(np.abs(fft_denoise(x[:, l])).max(axis=1) > 0)


@pytest.mark.parametrize("L", [256, 1000])
def test_ecg_like_inputs_match_the_restatement(L):
    from ecg_denoise_amd import fft_denoise
    x = U.ecg_like(L, 32)
    y, kept = fft_denoise(x, return_kept=True)
    ok = _check(x, y, kept, min_margin=5e-4, what=f"ecg-like L={L}")
    assert (~ok).sum() <= 8                                 # at most a quarter may be too close to the cutoff to compare


def test_properties_at_4096_rows_of_512():
    from ecg_denoise_amd import _lib, fft_denoise
    xn = U.designed(4096, (1.0,), 512, seed=21).reshape(4096, 512)
    x = torch.from_numpy(xn).to(DEV)
    y, kept = fft_denoise(x, return_kept=True)
    assert y.is_cuda and y.dtype == torch.float32 and kept.dtype == torch.int32 and kept.shape == (4096,)
    rows = np.arange(0, 4096, 257)
    _check(xn[rows], y[rows].cpu().numpy(), kept[rows].cpu().numpy(), what="4096 x 512, sampled")
    # two runs give the same bits
    y_again, kept_again = fft_denoise(x, return_kept=True)
    assert torch.equal(y.view(torch.int32), y_again.view(torch.int32)) and torch.equal(kept, kept_again)
    # linear in scale
    y4 = fft_denoise(4.0 * x)
    assert float((y4 - 4.0 * y).norm() / (4.0 * y).norm()) < 1e-6
    # threshold 0 keeps everything
    y0, kept0 = fft_denoise(x, threshold=0.0, return_kept=True)
    assert float((y0 - x).norm() / x.norm()) < 1e-6 and bool((kept0 == 512).all())
    # above 1 nothing survives; an all-zero group stays zero with every bin kept (nothing is below a cutoff of 0)
    y2, kept2 = fft_denoise(x[:8], threshold=1.5, return_kept=True)
    assert not bool(y2.any()) and not bool(kept2.any())
    yz, keptz = fft_denoise(torch.zeros(3, 2, 512, device=DEV), return_kept=True)
    assert not bool(yz.any()) and keptz.tolist() == [1024] * 3
    # threshold 1: the maximal bin (and its mirror) survives
    _, kept1 = fft_denoise(x[:64], threshold=1.0, return_kept=True)
    assert bool((kept1 >= 1).all()) and bool((kept1 <= 2).all())
    # in place equals out of place bit for bit
    z = x.clone()
    _lib.check(_lib.lib().ral_fft_denoise(C.c_void_p(z.data_ptr()), C.c_void_p(z.data_ptr()), None, 4096, 1, 512, U.THRESHOLD, None,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert torch.equal(z.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize("L,leads", [(1024, 12), (8192, 12), (8192, 2), (375, 2)])
def test_groups_in_place_and_repeatable(L, leads):
    """a resident group (one launch) and a group taken in two passes: in place equals out of place, two runs agree"""
    from ecg_denoise_amd import _lib, fft_denoise
    lib = _lib.lib()
    assert (lib.ral_fft_denoise_scratch_bytes(2, leads, L) > 0) == (L == 8192 and leads == 12)
    x = torch.from_numpy(U.designed(2, AMPS12[:leads], L, seed=L + leads)).to(DEV)
    y, kept = fft_denoise(x, return_kept=True)
    y_again, kept_again = fft_denoise(x, return_kept=True)
    assert torch.equal(y.view(torch.int32), y_again.view(torch.int32)) and torch.equal(kept, kept_again)
    z = x.clone()
    k2 = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    scratch = torch.empty(max(1, lib.ral_fft_denoise_scratch_bytes(2, leads, L)), dtype=torch.uint8, device=DEV)
    _lib.check(lib.ral_fft_denoise(C.c_void_p(z.data_ptr()), C.c_void_p(z.data_ptr()), C.c_void_p(k2.data_ptr()), 2, leads, L,
                                   U.THRESHOLD, C.c_void_p(scratch.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert torch.equal(z.view(torch.int32), y.view(torch.int32)) and torch.equal(k2, kept)


def test_raising_calls_leave_the_stream_usable():
    from ecg_denoise_amd import RalError, _lib, fft_denoise
    lib = _lib.lib()
    x = torch.from_numpy(U.designed(2, (1.0, 0.3), 256, seed=2)).to(DEV)
    y = torch.empty_like(x)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    px, py = C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr())
    for args, msg in (((None, py, None, 2, 2, 256, 0.04, None, s), b"null pointer"),
                      ((px, None, None, 2, 2, 256, 0.04, None, s), b"null pointer"),
                      ((px, py, None, -1, 2, 256, 0.04, None, s), b"groups=-1"),
                      ((px, py, None, 2, 0, 256, 0.04, None, s), b"rows_per_group=0"),
                      ((px, py, None, 2, 2, 1026, 0.04, None, s), b"L=1026"),
                      ((px, py, None, 2, 2, 8194, 0.04, None, s), b"L=8194"),
                      ((px, py, None, 2, 2, 256, -1.0, None, s), b"non-negative"),
                      ((px, py, None, 2, 2, 256, float("nan"), None, s), b"non-negative"),
                      ((px, py, None, 2, 12, 8192, 0.04, None, s), b"null scratch")):
        assert lib.ral_fft_denoise(*args) != 0 and msg in lib.ral_last_error(), (msg, lib.ral_last_error())
    assert lib.ral_fft_denoise(px, py, None, 0, 2, 256, 0.04, None, s) == 0          # no groups: nothing to do
    for bad in (x[0, 0], torch.zeros(2, 1026, device=DEV)):
        with pytest.raises(ValueError):
            fft_denoise(bad)
    with pytest.raises(ValueError):
        fft_denoise(x, threshold=-1.0)
    yv, kept = fft_denoise(x, return_kept=True)
    _check(x.cpu().numpy(), yv.cpu().numpy(), kept.cpu().numpy(), what="after the refusals")


def test_numpy_and_tensor_paths():
    """the rules of `wavelet_denoise`: NumPy in -> NumPy out in the input's float dtype (fp64 for integers), a device tensor in ->
    an fp32 device tensor out; a list of 1-D arrays is np.array(list)"""
    from ecg_denoise_amd import fft_denoise
    x = U.designed(3, (1.0, 0.3), 360, seed=3)
    y = fft_denoise(x)
    assert isinstance(y, np.ndarray) and y.dtype == np.float32 and y.shape == x.shape
    y64 = fft_denoise(x.astype(np.float64))
    assert y64.dtype == np.float64 and np.array_equal(y64.astype(np.float32), y)
    yt = fft_denoise(torch.from_numpy(x).to(DEV))
    assert torch.is_tensor(yt) and yt.is_cuda and yt.dtype == torch.float32 and np.array_equal(yt.cpu().numpy(), y)
    yd = fft_denoise(torch.from_numpy(x).to(DEV).double())
    assert yd.dtype == torch.float32 and torch.equal(yd, yt)
    xi = np.round(100 * x[:, 0]).astype(np.int16)
    yi = fft_denoise(xi)
    assert yi.dtype == np.float64 and yi.shape == xi.shape
    rows = [r for r in x[:, 0]]
    yl, kl = fft_denoise(rows, return_kept=True)
    assert isinstance(yl, np.ndarray) and isinstance(kl, np.ndarray) and np.array_equal(yl, fft_denoise(x[:, 0]))


@pytest.mark.parametrize("kind,L", [("fft", 1000), ("fft", 375), ("wavelet", 512)])
def test_classical_denoiser_equals_the_hand_cut_windows(kind, L):
    from ecg_denoise_amd import ClassicalDenoiser, fft_denoise, wavelet_denoise
    from ecg_denoise_amd import synth
    T = 5 * L // 2
    rec = torch.from_numpy(synth.make_records(2, 2, T, seed=6) + 0.3 * synth.make_noise_record("ma", 2, T, seed=8)).float().to(DEV)
    out = ClassicalDenoiser(kind, L, device=DEV).denoise(rec)
    assert out.shape == rec.shape and out.is_cuda
    want = torch.empty_like(rec)
    tail = T % L
    for r in range(2):
        for s in U.window_starts(T, L):
            w = rec[r:r + 1, :, s:s + L].contiguous()
            d = fft_denoise(w) if kind == "fft" else wavelet_denoise(w.reshape(2, L)).reshape(1, 2, L)
            if s + L == T and tail:
                want[r, :, T - tail:] = d[0, :, L - tail:]
            else:
                want[r, :, s:s + L] = d[0]
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    out_np = ClassicalDenoiser(kind, L, device=DEV).denoise(rec.cpu().numpy())
    assert isinstance(out_np, np.ndarray) and np.array_equal(out_np, out.cpu().numpy())


def test_classical_denoiser_stands_in_for_a_streaming_denoiser():
    """test_cls.py's question of the classical baselines, asked of the deterministic detector and classifier"""
    from ecg_denoise_amd import ClassicalDenoiser, evaluate_beats, evaluate_rhythm, synth
    T = 6000
    x, truth, labels = synth.make_records_with_rhythm(3, 2, T, seed=14, p_v=0.12, p_s=0.08)
    rec = torch.from_numpy(x).to(DEV)
    noise = torch.from_numpy(synth.make_noise_record("emb", 2, T + 500, seed=3)).to(DEV)
    for kind, L in (("fft", 1000), ("wavelet", 1024)):
        dn = ClassicalDenoiser(kind, L, device=DEV)
        eb = evaluate_beats(dn, rec, noise, 0.0, offsets=[5, 200, 499])
        assert all(np.isfinite(v) for v in eb.denoised.pooled.values()) and eb.denoised.pooled["tp"] > 0
        er = evaluate_rhythm(dn, rec, noise, 0.0, ref=truth, ref_labels=labels, offsets=[5, 200, 499])
        assert np.isfinite(er.scores["denoised"]["acc"]) and 0.0 <= er.scores["denoised"]["acc"] <= 1.0
        assert np.isfinite(er.scores["noisy"]["acc"])
