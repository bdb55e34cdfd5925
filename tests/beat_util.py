"""The numpy oracle of the beat detector (include/ralenet.h, "beat detection"; ecg_denoise_amd/beats.py): an fp64 restatement of
the definition, the three margins that say how far every decision of a record lies from a tie, the matching walk, and the
inputs that the CPU guard and the GPU tests share.

The restatement follows the definition line by line and in its order (taps ascending, leads in lead order, the integrator's
terms ascending); `dtype=np.float32` runs the same statements in fp32 (products and sums rounded separately: numpy has no fused
multiply-add)."""
import functools
from fractions import Fraction

import numpy as np

ALPHA, FLOOR, BAND = 0.35, 0.0, (8, 24)


def _round(v):
    """nearest integer, halves up, in exact rational arithmetic"""
    return int((Fraction(v) + Fraction(1, 2)).__floor__())


def geometry(fs):
    fs = Fraction(fs)
    return {"half": _round(fs / 4), "Wi": _round(fs * 3 / 40), "Wt": _round(fs * 3 / 2), "Rf": _round(fs / 5),
            "Rw": _round(fs * 3 / 40)}


def bank(fs, f_lo=BAND[0], f_hi=BAND[1]):
    half = geometry(fs)["half"]
    fs = float(Fraction(fs))
    k = np.arange(-half, half + 1, dtype=np.float64)
    h = ((2 * f_hi / fs) * np.sinc(2 * f_hi * k / fs) - (2 * f_lo / fs) * np.sinc(2 * f_lo * k / fs)) * np.hamming(2 * half + 1)
    return h - h.mean()


def frontier(n_in, fs):
    g = geometry(fs)
    return max(0, int(n_in) - (g["Wt"] + g["Wi"] + g["half"]))


def features(x, fs=360, band=BAND, dtype=np.float64):
    """x (leads, T) -> (f, m), each (T,) of `dtype`"""
    g = geometry(fs)
    half, Wi = g["half"], g["Wi"]
    h = bank(fs, *band).astype(np.float32).astype(dtype)          # the taps the device gets
    x = np.asarray(x, dtype=np.float32).astype(dtype)
    leads, T = x.shape
    f = np.zeros(T, dtype=dtype)
    for l in range(leads):
        xp = np.concatenate([np.full(half, x[l, 0], dtype), x[l], np.full(half, x[l, -1], dtype)])   # xp[i] = x[clamp(i - half)]
        y = np.zeros(T, dtype=dtype)
        for k in range(-half, half + 1):                           # x[clamp(n - k)] = xp[n - k + half]
            y = y + h[k + half] * xp[half - k:half - k + T]
        f = f + y * y
    fp = np.concatenate([np.zeros(Wi, dtype), f, np.zeros(Wi, dtype)])
    s = np.zeros(T, dtype=dtype)
    for j in range(2 * Wi + 1):
        s = s + fp[j:j + T]
    return f, s / dtype(2 * Wi + 1)


def _window_max(v, before, after, fill):
    """max of v[n - before .. n + after] clipped to the array, for every n (`fill` where the window is empty)"""
    T = len(v)
    if before + after + 1 <= 0:
        return np.full(T, fill, dtype=v.dtype)
    p = np.concatenate([np.full(max(before, 0), fill, v.dtype), v, np.full(max(after, 0), fill, v.dtype)])
    w = np.lib.stride_tricks.sliding_window_view(p, before + after + 1)
    return w.max(axis=1)[:T]


def _refractory(m, Rf):
    """n with m[n] > 0, m[n] > m[n + j] for -Rf <= j < 0 and m[n] >= m[n + j] for 0 < j <= Rf (clipped)"""
    T = len(m)
    left = np.full(T, -np.inf)
    right = np.full(T, -np.inf)
    if T > 1:
        left[1:] = _window_max(m[:-1].astype(np.float64), Rf - 1, 0, -np.inf)     # max of m[n - Rf .. n - 1]
        right[:-1] = _window_max(m[1:].astype(np.float64), 0, Rf - 1, -np.inf)    # max of m[n + 1 .. n + Rf]
    return (m > 0) & (m > left) & (m >= right)


def detect(x, fs=360, alpha=ALPHA, floor=FLOOR, band=BAND, dtype=np.float64, margins=False):
    """x (leads, T) -> the peaks of one record, ascending (a list of ints); with margins=True also a dict of the three margins
    (inf where a record offers nothing to measure)"""
    g = geometry(fs)
    f, m = features(x, fs, band, dtype)
    T = len(m)
    thr = np.maximum(dtype(alpha) * _window_max(m, g["Wt"], g["Wt"], dtype(-1)), dtype(floor))
    local = _refractory(m, g["Rf"])
    cand = np.flatnonzero(local & (m >= thr))
    peaks, gap, edge = [], np.inf, np.inf
    for n in cand:
        lo, hi = max(0, n - g["Rw"]), min(T - 1, n + g["Rw"])
        w = f[lo:hi + 1]
        p = lo + int(np.argmax(w))                                  # (the lowest index that attains the maximum)
        peaks.append(p)
        if len(w) > 1:
            gap = min(gap, float((w.max() - np.delete(w, p - lo).max()) / w.max()))
        edge = min(edge, p - (n - g["Rw"]), (n + g["Rw"]) - p)
    if not margins:
        return peaks
    at = np.flatnonzero(local & (thr > 0))
    rel = float(np.min(np.abs(m[at] - thr[at]) / thr[at])) if len(at) else np.inf
    return peaks, {"threshold": rel, "top": gap, "edge": edge}


def detect_records(x, **kw):
    return [detect(r, **kw) for r in np.asarray(x)]


def match(ref, det, tol):
    """the walk over two sorted lists -> (tp, fp, fn): ref[i] and det[j] match iff |det - ref| <= tol, otherwise the smaller
    index advances (a detection before its reference is a false positive, a reference before its detection a miss)"""
    i = j = tp = fp = fn = 0
    while i < len(ref) and j < len(det):
        if abs(det[j] - ref[i]) <= tol:
            tp, i, j = tp + 1, i + 1, j + 1
        elif det[j] < ref[i]:
            fp, j = fp + 1, j + 1
        else:
            fn, i = fn + 1, i + 1
    return tp, fp + len(det) - j, fn + len(ref) - i


# ---------------------------------------------------------------------------------------------- the shared inputs
SHAPES = ((5, (4, 2, 1440)), (6, (3, 1, 2000)), (7, (3, 2, 3000)))      # (make_records seed, (R, leads, T))
NOISE_DB = (None, 6.0, 0.0)                                             # clean, emb at 6 dB, emb at 0 dB


def zscore(x):
    x = np.asarray(x, dtype=np.float64)
    return (x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True)


def add_noise(clean, z, snr_db):
    """clean (R, leads, T) + z (leads, T) scaled per record to `snr_db` (powers over all leads and samples of the record)"""
    p_sig = (clean ** 2).mean((1, 2), keepdims=True)
    p_noise = (z ** 2).mean()
    return clean + np.sqrt(p_sig / 10 ** (snr_db / 10) / p_noise) * z[None]


@functools.lru_cache(maxsize=None)
def inputs():
    """-> ((name, float32 (R, leads, T)), ...): the records of SHAPES z-scored, clean and with `emb` noise at 6 and 0 dB;
    30 records in 9 groups"""
    from ecg_denoise_amd import synth
    out = []
    for seed, (R, leads, T) in SHAPES:
        clean = zscore(synth.make_records(R, leads, T, seed=seed))
        z = synth.make_noise_record("emb", leads, T, seed=seed + 100).astype(np.float64)
        for db in NOISE_DB:
            x = clean if db is None else add_noise(clean, z, db)
            out.append((f"seed{seed}_{R}x{leads}x{T}_{'clean' if db is None else f'emb{db:g}dB'}", x.astype(np.float32)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected():
    """-> {name: [peaks of each record]} of `inputs()`, from the fp64 restatement"""
    return {name: detect_records(x) for name, x in inputs()}
