"""The FFT-threshold baseline restated in fp64 (local_utils/denoisefunc.py:36-66; the reference function itself cannot run: it
never imports `fft` / `ifft`, so there is no reference-generated golden), and the inputs the tests use.

    X = fft(item);  mag = |X|;  cutoff = threshold * max(mag);  X[mag < cutoff] = 0;  out = ifft(X).real

per item of the first axis, `fft` / `ifft` being numpy's along the last axis: a row of a 2-D array is thresholded against its own
maximum, the leads of an item of a 3-D array against one maximum."""
import numpy as np

GOLDEN_LENGTHS = (16, 30, 112, 1000)
GOLDEN_AMPS = (1.0, 0.3, 0.02)
GOLDEN_GROUPS = 2
THRESHOLD = 0.04


def fft_denoise_ref(x, threshold=THRESHOLD):
    """-> (out fp64 of x's shape, kept (groups,) int64, margin (groups,)).  The margin of a group is min |mag - cutoff| / cutoff
    over its bins (inf when the cutoff is 0): how far the nearest bin is from changing sides."""
    x = np.asarray(x, dtype=np.float64)
    assert x.ndim in (2, 3)
    out, kept, margin = np.empty_like(x), [], []
    for i, item in enumerate(x):
        X = np.fft.fft(item)
        mag = np.abs(X)
        cutoff = threshold * np.max(mag)
        X[mag < cutoff] = 0
        out[i] = np.fft.ifft(X).real
        kept.append(int(np.count_nonzero(~(mag < cutoff))))
        margin.append(float(np.min(np.abs(mag - cutoff)) / cutoff) if cutoff > 0 else np.inf)
    return out, np.array(kept, dtype=np.int64), np.array(margin)


def designed(groups, amps, L, seed, threshold=THRESHOLD):
    """-> float32 (groups, len(amps), L) whose bins all lie far from the cutoff: per lead a random Hermitian spectrum with
    uniform random phases; bin levels relative to the group's maximum half from [0.001, 0.75 thr] and half from
    [1.25 thr, amp of the lead] (a lead whose amp is below 1.25 thr: the low part only); one bin of lead 0 at 1.  The signal is
    the fp64 irfft times sqrt(L), rounded to fp32."""
    rng = np.random.default_rng(seed)
    leads, nb = len(amps), L // 2 + 1
    lo, hi = 0.75 * threshold, 1.25 * threshold
    level = np.empty((groups, leads, nb))
    for l, amp in enumerate(amps):
        low = rng.uniform(0.001, lo, (groups, nb))
        if amp >= hi:
            level[:, l] = np.where(rng.random((groups, nb)) < 0.5, low, rng.uniform(hi, amp, (groups, nb)))
        else:
            level[:, l] = low
    level[np.arange(groups), 0, rng.integers(0, nb, groups)] = 1.0
    phase = rng.uniform(0, 2 * np.pi, (groups, leads, nb))
    phase[..., 0] = np.pi * rng.integers(0, 2, (groups, leads))           # real bins: DC ...
    if L % 2 == 0:
        phase[..., -1] = np.pi * rng.integers(0, 2, (groups, leads))      # ... and L / 2
    spec = level * np.exp(1j * phase)
    spec[..., 0] = spec[..., 0].real
    if L % 2 == 0:
        spec[..., -1] = spec[..., -1].real
    return (np.fft.irfft(spec, n=L, axis=-1) * np.sqrt(L)).astype(np.float32)


def ecg_like(L, n):
    """-> float32 (n, 2, L): synthetic two-lead ECG with muscle artefact, cut into n items"""
    from ecg_denoise_amd import synth
    T = n * L // 2
    x = synth.make_records(2, 2, T, seed=11) + 0.5 * synth.make_noise_record("ma", 2, T, seed=3)
    return np.ascontiguousarray(x.reshape(2, 2, n // 2, L).transpose(0, 2, 1, 3).reshape(n, 2, L), dtype=np.float32)


def rel_l2(y, ref):
    """per group: ||y - ref|| / ||ref|| (the absolute norm where ref is zero)"""
    y, ref = np.asarray(y, np.float64).reshape(len(ref), -1), np.asarray(ref, np.float64).reshape(len(ref), -1)
    den = np.linalg.norm(ref, axis=1)
    return np.linalg.norm(y - ref, axis=1) / np.where(den > 0, den, 1.0)


def window_starts(T, L):
    """`StreamingDenoiser.window_starts` at overlap 0"""
    return [k * L for k in range(T // L)] + ([T - L] if T % L else [])
