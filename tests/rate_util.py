"""The sample-rate conversion of ecg_denoise_amd.rate restated in fp64 numpy, independently of the package: the oracle of the
rate tests.  scipy.signal.resample_poly(x, up, down, window=('kaiser', 5.0), padtype='edge') agrees with it to 1e-16
(tests/golden/g9_rate.npz holds scipy's results)."""
from fractions import Fraction

import numpy as np

# the fixture's cases: (fs_in, fs_out) -> record lengths
PAIRS = [(500, 360), (250, 360), (1000, 360), (128, 360), (257, 360), (360, 500), (360, 250), (360, 128)]
LENGTHS = {p: (1, 7, 700) + ((1531,) if p in ((500, 360), (360, 500)) else ()) for p in PAIRS}
LEADS = 2
# every rate the package supports next to 360 Hz
RATES = (100, 125, 128, 200, 250, 256, 257, 300, 400, 500, 512, 1000, 1024)


def ratio(fs_in, fs_out):
    q = Fraction(fs_out, fs_in)
    return q.numerator, q.denominator


def bank(up, down):
    mx = max(up, down)
    half = 10 * mx
    k = np.arange(-half, half + 1)
    h = (1.0 / mx) * np.sinc(k / mx) * np.kaiser(2 * half + 1, 5.0)
    return h * (up / h.sum())


def length(T, up, down):
    return (T * up + down - 1) // down


def convert(x, up, down, h=None, dtype=np.float64):
    """x (..., T) -> (..., ceil(T up / down)); the sum over n ascending.  dtype float32: every product and sum rounded to fp32
    one after the other (what a device without fused multiply-add would give; fmaf rounds once per tap instead of twice)"""
    x = np.asarray(x, dtype=dtype)
    h = (bank(up, down) if h is None else np.asarray(h)).astype(dtype)
    T, half = x.shape[-1], 10 * max(up, down)
    y = np.zeros(x.shape[:-1] + (length(T, up, down),), dtype=dtype)
    for m in range(y.shape[-1]):
        lo, hi = -((half - m * down) // up), (m * down + half) // up
        acc = np.zeros(x.shape[:-1], dtype=dtype)
        for n in range(lo, hi + 1):
            acc = acc + h[m * down - n * up + half] * x[..., min(max(n, 0), T - 1)]
        y[..., m] = acc
    return y


def adc_records(R, leads, T, seed):
    """ADC-like integer samples (as wfdb's d_signal): baseline 1024, a slow wave and noise, different per record and lead"""
    rng = np.random.default_rng(seed)
    t = np.arange(T)[None, None, :]
    amp = rng.uniform(100, 400, (R, leads, 1))
    x = 1024 + amp * np.sin(t / rng.uniform(30, 90, (R, leads, 1))) + 60 * rng.standard_normal((R, leads, T))
    return x.astype(np.int32).astype(np.float64)
