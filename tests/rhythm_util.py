"""The numpy oracle of the beat classifier (include/ralenet.h, "beat classes"; ecg_denoise_amd/rhythm.py): an fp64 restatement
of the definition, one beat at a time and sample by sample where the kernel works in parallel, the tolerances of the GPU
comparison, and the comparison itself."""
from fractions import Fraction

import numpy as np

K, MIN_REF, C0, R0 = 8, 3, 0.7, 0.8
EPS = 2.0 ** -24


def _round(v):
    """nearest integer, halves up, in exact rational arithmetic"""
    return int((Fraction(v) + Fraction(1, 2)).__floor__())


def geometry(fs):
    fs = Fraction(fs)
    return {"Wb": _round(fs / 10), "Sa": _round(fs / 120)}


def hood(i, n):
    """the beats [a, hi) that beat i of n is judged among (beat i is one of them)"""
    a = min(max(i - K, 0), max(0, n - K - 1))
    return a, min(n, a + K + 1)


def window(x, p, Wb):
    """x (leads, T) -> (leads, 2 Wb + 1): x_l[clamp(p + k, 0, T - 1)], k = -Wb .. Wb, minus the window's own mean per lead"""
    leads, T = x.shape
    w = np.empty((leads, 2 * Wb + 1), dtype=np.float64)
    for l in range(leads):
        for k in range(-Wb, Wb + 1):
            w[l, k + Wb] = x[l, min(max(p + k, 0), T - 1)]
        w[l] -= w[l].sum() / (2 * Wb + 1)
    return w


def classify_beat(x, pos, i, fs=360, c0=C0, r0=R0):
    """beat i of the record x (leads, T) with the beats `pos` -> (label, corr, rr_ratio) in fp64"""
    g = geometry(fs)
    Wb, Sa = g["Wb"], g["Sa"]
    x = np.asarray(x, dtype=np.float64)
    n = len(pos)
    a, hi = hood(i, n)
    nb = [j for j in range(a, hi) if j != i]
    if len(nb) < MIN_REF:
        return -1, float("nan"), float("nan")
    t = np.median(np.stack([window(x, int(pos[j]), Wb) for j in nb]), axis=0)
    corr = None
    for s in range(-Sa, Sa + 1):
        v = window(x, int(pos[i]) + s, Wb)
        den = float((t * t).sum() * (v * v).sum())
        c = float((t * v).sum() / np.sqrt(den)) if den > 0 else 0.0
        corr = c if corr is None or c > corr else corr
    if i == 0:
        rr = float("nan")
    else:
        rr = float((int(pos[i]) - int(pos[i - 1])) / np.median(np.diff(np.asarray(pos[a:hi], dtype=np.int64)).astype(np.float64)))
    label = 1 if corr < c0 else (2 if i > 0 and rr < r0 else 0)
    return label, corr, rr


def classify_record(x, pos, **kw):
    """-> (labels, corr, rr_ratio): three lists, one value per beat"""
    out = [classify_beat(x, pos, i, **kw) for i in range(len(pos))]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


def corr_tol(leads, fs):
    """absolute: three dot products of n = leads (2 Wb + 1) terms in fp32 under a normalisation, sum |a b| <= sqrt(sum a^2
    sum b^2): 4 n 2^-24"""
    return 4 * leads * (2 * geometry(fs)["Wb"] + 1) * EPS


RR_TOL = 4 * EPS          # relative


def near_threshold(corr, rr, i, leads, fs, c0=C0, r0=R0):
    """the oracle's corr or rr_ratio lies within its tolerance of its threshold: the label may differ there"""
    return abs(corr - c0) <= corr_tol(leads, fs) or (i > 0 and abs(rr - r0) <= RR_TOL * abs(rr))


def compare(x, pos, got, fs=360, c0=C0, r0=R0):
    """x (leads, T), pos, got = (labels, corr, rr_ratio) of the device for this record -> the number of beats whose label was
    exempt from the comparison; asserts everything else"""
    leads = x.shape[0]
    lab, corr, rr = classify_record(x, pos, fs=fs, c0=c0, r0=r0)
    assert len(got[0]) == len(got[1]) == len(got[2]) == len(pos)
    exempt = 0
    for i in range(len(pos)):
        where = f"beat {i} of {len(pos)}: device {got[0][i], got[1][i], got[2][i]}, oracle {lab[i], corr[i], rr[i]}"
        if lab[i] < 0:
            assert got[0][i] == -1 and np.isnan(got[1][i]) and np.isnan(got[2][i]), where
            continue
        assert abs(got[1][i] - corr[i]) <= corr_tol(leads, fs), where
        if i == 0:
            assert np.isnan(got[2][i]) and np.isnan(rr[i]), where
        else:
            assert abs(got[2][i] - rr[i]) <= RR_TOL * abs(rr[i]), where
        if near_threshold(corr[i], rr[i], i, leads, fs, c0, r0):
            exempt += 1
        else:
            assert got[0][i] == lab[i], where
    return exempt
