"""CPU checks of the FFT-threshold baseline: the fp64 restatement (tests/fft_util.py) against its golden and its own
properties, the designed inputs' distance from the cutoff, and everything of the library and the host mirror that needs no
device - the ABI table, the length rule, the refusals of `fft_denoise`, the windows of `ClassicalDenoiser`."""
import os

import numpy as np
import pytest

import fft_util as U


def test_restatement_matches_the_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "g10_fft.npz"))
    assert float(g["threshold"]) == U.THRESHOLD
    for L in U.GOLDEN_LENGTHS:
        x = g[f"x_{L}"]
        assert x.dtype == np.float32 and x.shape == (U.GOLDEN_GROUPS, len(U.GOLDEN_AMPS), L)
        assert np.array_equal(x, U.designed(U.GOLDEN_GROUPS, U.GOLDEN_AMPS, L, seed=1000 + L))
        y, kept, margin = U.fft_denoise_ref(x)
        assert np.abs(y - g[f"y_{L}"]).max() < 1e-12 and np.array_equal(kept, g[f"kept_{L}"]) and margin.min() >= 1e-2
        y2, kept2, _ = U.fft_denoise_ref(x.reshape(-1, L))
        assert np.abs(y2 - g[f"y2_{L}"]).max() < 1e-12 and np.array_equal(kept2, g[f"kept2_{L}"])
        # the 0.02 lead: nothing of it survives the group rule, something does when its row stands alone
        assert np.array_equal(y[:, 2], np.zeros_like(y[:, 2])) and np.all(np.abs(y2[2::3]).max(axis=1) > 0)


@pytest.mark.parametrize("L", [16, 17, 30, 112])
def test_kept_set_is_hermitian_and_counts_the_full_spectrum(L):
    x = U.designed(3, (1.0, 0.3), L, seed=L)
    _, kept, _ = U.fft_denoise_ref(x)
    for item, k in zip(x.astype(np.float64), kept):
        mag = np.abs(np.fft.fft(item))
        keep = ~(mag < U.THRESHOLD * mag.max())
        assert np.array_equal(keep[:, 1:], keep[:, :0:-1])                  # bin j and bin L - j fall together
        half = keep[:, :L // 2 + 1]
        w = np.full(L // 2 + 1, 2)
        w[0] = 1
        if L % 2 == 0:
            w[-1] = 1
        assert int((half * w).sum()) == k == int(keep.sum())


def test_threshold_zero_is_identity_and_above_one_gives_zeros():
    x = U.designed(2, (1.0, 0.3), 112, seed=5)
    y0, kept0, m0 = U.fft_denoise_ref(x, 0.0)
    assert np.abs(y0 - x).max() < 1e-12 and np.all(kept0 == 2 * 112) and np.all(np.isinf(m0))
    y1, kept1, _ = U.fft_denoise_ref(x, 1.0)                                # `<`: the maximal bin survives threshold = 1
    assert np.all(kept1 >= 1) and np.all(np.abs(y1).max(axis=(1, 2)) > 0)
    y2, kept2, _ = U.fft_denoise_ref(x, 1.5)
    assert np.array_equal(y2, np.zeros_like(y2)) and np.all(kept2 == 0)
    z, keptz, _ = U.fft_denoise_ref(np.zeros((2, 16)))
    assert np.array_equal(z, np.zeros((2, 16))) and np.all(keptz == 16)     # cutoff 0: nothing is below it


def test_a_3d_item_differs_from_its_rows_taken_as_2d():
    x = U.designed(2, (1.0, 0.3, 0.02), 256, seed=9)
    y3, kept3, _ = U.fft_denoise_ref(x)
    y2, kept2, _ = U.fft_denoise_ref(x.reshape(-1, 256))
    assert np.abs(y3 - y2.reshape(x.shape)).max() > 1e-3 and kept2.reshape(2, 3).sum(axis=1).tolist() != kept3.tolist()
    same = U.designed(2, (1.0,), 256, seed=9)                               # one lead: the two readings coincide
    assert np.array_equal(U.fft_denoise_ref(same)[0].reshape(2, 256), U.fft_denoise_ref(same.reshape(2, 256))[0])


@pytest.mark.parametrize("L", [2, 16, 17, 18, 20, 30, 112, 256, 360, 375, 512, 1000, 1008, 1022, 1024, 7680, 8192])
def test_designed_inputs_keep_their_distance_from_the_cutoff(L):
    for groups, amps in ((1, (1.0,)), (3, (1.0, 0.3)), (2, (1.0, 0.3, 0.02)), (5, (1.0,))):
        x = U.designed(groups, amps, L, seed=L + len(amps))
        assert x.dtype == np.float32 and x.shape == (groups, len(amps), L)
        assert U.fft_denoise_ref(x)[2].min() >= 1e-2


def test_ecg_like_inputs():
    for L, skipped in ((256, 0), (1000, 3)):
        x = U.ecg_like(L, 32)
        assert x.shape == (32, 2, L) and x.dtype == np.float32
        assert int((U.fft_denoise_ref(x)[2] < 5e-4).sum()) <= 8


def test_lib_declares_both_entry_points():
    from ecg_denoise_amd import _lib
    assert "ral_fft_denoise" in _lib.EXPORTS and "ral_fft_denoise_scratch_bytes" in _lib.EXPORTS
    L = _lib.lib()
    assert L.ral_fft_denoise.argtypes[3] is __import__("ctypes").c_int64 and len(L.ral_fft_denoise.argtypes) == 9


def _rule(L):
    m = L
    for f in (2, 3, 5):
        while m > 1 and m % f == 0:
            m //= f
    fast = L % 2 == 0 and m == 1 and 16 <= L <= 8192
    return fast or 2 <= L <= 1024


def test_scratch_bytes_accepts_and_refuses_exactly_the_lengths_of_the_rule():
    from ecg_denoise_amd import _lib
    L = _lib.lib()
    f = L.ral_fft_denoise_scratch_bytes
    for n in list(range(-2, 1300)) + list(range(8000, 8300)) + [2048, 2050, 2187, 2250, 3000, 3125, 4374, 6250, 7680, 7777, 1 << 20]:
        assert (f(1, 1, n) >= 0) == _rule(n), n
    assert f(1, 1, 1026) < 0 and b"L=1026" in L.ral_last_error() and b"prime factor" in L.ral_last_error()
    for n in (1026, 1125, 8194, 1, 0):
        assert f(1, 1, n) < 0
    # resident groups need no scratch (2 x 8192 and 12 x 1024 fit LDS), 12 x 8192 takes two passes: 4 bytes per row
    assert f(7, 2, 8192) == 0 and f(7, 12, 1024) == 0 and f(7, 1, 1008) == 0 and f(0, 1, 256) == 0
    assert f(7, 12, 8192) == 7 * 12 * 4 and f(3, 400, 1008) == 3 * 400 * 4
    assert f(-1, 1, 256) < 0 and b"groups" in L.ral_last_error()
    assert f(1, 0, 256) < 0 and f(1 << 31, 2, 256) < 0
    # argument errors of the compute entry point that are found before any device work
    g = L.ral_fft_denoise
    assert g(None, None, None, 1, 1, 256, 0.04, None, None) != 0 and b"null pointer" in L.ral_last_error()


def test_fft_denoise_raises_before_any_device_work():
    from ecg_denoise_amd import fft_denoise
    z = lambda *s: np.zeros(s, np.float32)
    for bad in (z(256), [z(16), z(18)], z(2, 1026), z(2, 1125), z(2, 8194), z(2, 3, 1026), z(2, 2, 2, 16)):
        with pytest.raises(ValueError):
            fft_denoise(bad)
    for thr in (-1, float("nan")):
        with pytest.raises(ValueError):
            fft_denoise(z(2, 256), threshold=thr)


def test_classical_denoiser_windows():
    from ecg_denoise_amd import ClassicalDenoiser, RalError
    for kind, L in (("fft", 1000), ("fft", 375), ("wavelet", 512)):
        d = ClassicalDenoiser(kind, L)
        assert d.window_starts(5 * L // 2) == U.window_starts(5 * L // 2, L) == [0, L, 5 * L // 2 - L]
        assert d.window_starts(L) == [0] and d.window_starts(2 * L) == [0, L]
        with pytest.raises(RalError):
            d.window_starts(L - 1)
        with pytest.raises(RalError):
            d.denoise(np.zeros((1, 2, L - 1), np.float32))
        assert not hasattr(d, "fs")                                         # the evaluations then take the model rate, 360 Hz
    for kw in (dict(kind="median", L=256), dict(kind="fft", L=1026), dict(kind="wavelet", L=511), dict(kind="fft", L=256, threshold=-1)):
        with pytest.raises(ValueError):
            ClassicalDenoiser(**kw)
