"""The HRV definition of include/ralenet.h restated in numpy, and the tolerances of the device results against it.

    oracle(pos, lab, w0, w1, g)        one window in fp64 (exact integers first) -> dict
    oracle_record(pos, lab, T, g)      every window of a record
    emulate_psd(q, d, g)               the spectrum in fp32 with sequential sums: what the kernel's arithmetic can attain
    compare(got, want, g)              the tolerances below; -> the worst spectral error as a fraction of its bound

Tolerances.  counts: exact.  Time domain: 4 * 2^-24 relative (exact integers, then a few fp64 operations: two fp32 ulps).
Per bin: |psd_k - oracle| <= 4 (16 + m) 2^-24 S with S = 2 sum y^2 / (m fs^2) from the oracle - the phase argument carries about
15 units of 2^-24, sequential accumulation m more, P <= sum y^2 and the denominators are about m / 2; the condition, asserted
with no exemptions, is min(cc, ss) >= m / 4 in the oracle.  Band sums: the sum of their bins' tolerances plus
n_bins 2^-24 |value|.  lf_hf: the quotient of the two returned values within 2^-23 relative."""
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -24
STATS = ("mean_nn", "hr", "sdnn", "rmssd", "pnn50", "vlf", "lf", "hf", "total", "lf_hf")


def nn_intervals(pos, lab, w0, w1, g):
    """-> (beats, q, d, index i of every NN interval) of the window [w0, w1)"""
    pos = np.asarray(pos, dtype=np.int64)
    lab = np.zeros(len(pos), dtype=np.int64) if lab is None else np.asarray(lab, dtype=np.int64)
    inside = (pos >= w0) & (pos < w1)
    q, d, idx = [], [], []
    for i in range(1, len(pos)):
        di = int(pos[i] - pos[i - 1])
        if inside[i - 1] and inside[i] and lab[i - 1] == 0 and lab[i] == 0 and g["lo_n"] <= di <= g["hi_n"]:
            q.append(int(pos[i] - w0)), d.append(di), idx.append(i)
    return int(inside.sum()), q, d, idx


def spectrum64(q, d, g):
    """-> (psd (F,) fp64, S, min over the bins of min(cc, ss))"""
    m, fs, W, F = len(d), float(g["fs"]), g["W"], g["F"]
    S1 = sum(d)
    y = (np.asarray(d, dtype=np.float64) - S1 / m).astype(np.float32).astype(np.float64)
    k1 = np.arange(1, F + 1, dtype=np.int64)[:, None]
    r = (k1 * np.asarray(q, dtype=np.int64)[None, :]) % W
    ph = 2 * np.pi * r / W
    c, s = np.cos(ph), np.sin(ph)
    YC, YS, CC, SS, CS = (c * y).sum(1), (s * y).sum(1), (c * c).sum(1), (s * s).sum(1), (c * s).sum(1)
    th = 0.5 * np.arctan2(2 * CS, CC - SS)
    ct, st = np.cos(th), np.sin(th)
    yc, ys = ct * YC + st * YS, ct * YS - st * YC
    cc = ct * ct * CC + 2 * ct * st * CS + st * st * SS
    ss = ct * ct * SS - 2 * ct * st * CS + st * st * CC
    with np.errstate(divide="ignore", invalid="ignore"):
        P = 0.5 * (np.where(cc != 0, yc * yc / cc, 0.0) + np.where(ss != 0, ys * ys / ss, 0.0))
    return 2 * P / (m * fs * fs), 2 * float((y * y).sum()) / (m * fs * fs), float(np.minimum(cc, ss).min())


def emulate_psd(q, d, g):
    """the kernel's spectrum in numpy fp32: the argument fp32(2 r) / fp32(W) handed to an accurate sin / cos of pi x, fp32
    products added sequentially in j, the rotation and the quotient in fp32 -> psd (F,) fp32"""
    f32 = np.float32
    m, fs, W, F = len(d), float(g["fs"]), g["W"], g["F"]
    y = (np.asarray(d, dtype=np.float64) - sum(d) / m).astype(f32)
    k1 = np.arange(1, F + 1, dtype=np.int64)
    YC, YS, CC, SS, CS = (np.zeros(F, dtype=f32) for _ in range(5))
    for j in range(m):
        r = (k1 * q[j]) % W
        a = (2 * r).astype(f32) / f32(W)
        c, s = np.cos(np.pi * a.astype(np.float64)).astype(f32), np.sin(np.pi * a.astype(np.float64)).astype(f32)
        YC, YS, CC, SS, CS = YC + y[j] * c, YS + y[j] * s, CC + c * c, SS + s * s, CS + c * s
    th = f32(0.5) * np.arctan2(f32(2) * CS, CC - SS)
    ct, st = np.cos(th), np.sin(th)
    yc, ys = ct * YC + st * YS, ct * YS - st * YC
    x2 = f32(2) * ct * st * CS
    cc, ss = ct * ct * CC + x2 + st * st * SS, ct * ct * SS - x2 + st * st * CC
    with np.errstate(divide="ignore", invalid="ignore"):
        P = f32(0.5) * (np.where(cc != 0, yc * yc / cc, f32(0)) + np.where(ss != 0, ys * ys / ss, f32(0)))
    return (P * f32(2.0 / (m * fs * fs))).astype(f32)


def oracle(pos, lab, w0, w1, g):
    """one window -> {"counts": [beats, m, k, n50], "stats": (10,) fp64, "psd": (F,) fp64, "S", "m", "den": min(cc, ss)}"""
    fs = float(g["fs"])
    beats, q, d, idx = nn_intervals(pos, lab, w0, w1, g)
    m = len(d)
    deltas = [d[j] - d[j - 1] for j in range(1, m) if idx[j] == idx[j - 1] + 1]
    k, n50 = len(deltas), sum(abs(x) > g["t50"] for x in deltas)
    S1, S2, D2 = sum(d), sum(x * x for x in d), sum(x * x for x in deltas)          # Python integers: exact
    st = np.full(10, np.nan)
    if m >= 1:
        st[0], st[1] = S1 / (m * fs), 60.0 * m * fs / S1
    if m >= 2:
        st[2] = np.sqrt(float(Fraction(m * S2 - S1 * S1, m * (m - 1)))) / fs
    if k >= 1:
        st[3], st[4] = np.sqrt(D2 / k) / fs, n50 / k
    out = {"counts": [beats, m, k, n50], "stats": st, "psd": np.full(g["F"], np.nan), "S": np.nan, "m": m, "den": np.nan}
    if m >= g["min_nn"]:
        psd, S, den = spectrum64(q, d, g)
        for b in range(3):
            st[5 + b] = psd[g["band"] == b].sum()
        st[8] = psd.sum()
        with np.errstate(divide="ignore", invalid="ignore"):
            st[9] = np.float64(st[6]) / np.float64(st[7])
        out.update(psd=psd, S=S, den=den)
    return out


def windows(T, g):
    nw = max(1, (T - g["W"]) // g["H"] + 1)
    return [(w * g["H"], min(w * g["H"] + g["W"], T)) for w in range(nw)]


def oracle_record(pos, lab, T, g):
    return [oracle(pos, lab, w0, w1, g) for w0, w1 in windows(T, g)]


def bin_tol(o):
    return 4 * (16 + o["m"]) * EPS * o["S"]


def compare(counts, stats, psd, want, g):
    """one window of the device (counts (4,), stats (10,), psd (F,) or None, as numpy) against the oracle's `want` -> the worst
    spectral error of the window as a fraction of its bound (0.0 without a spectrum); prints nothing, asserts everything"""
    assert [int(v) for v in counts] == want["counts"], (counts, want["counts"])
    ws = want["stats"]
    for e in range(5):
        if np.isnan(ws[e]):
            assert np.isnan(stats[e]), (STATS[e], stats[e])
        else:
            assert abs(float(stats[e]) - ws[e]) <= 4 * EPS * abs(ws[e]), (STATS[e], stats[e], ws[e])
    if want["m"] < g["min_nn"]:
        assert all(np.isnan(stats[5:])) and (psd is None or np.all(np.isnan(psd)))
        return 0.0
    assert want["den"] >= want["m"] / 4, ("the condition of the spectral bound", want["den"], want["m"])
    tol, worst = bin_tol(want), 0.0
    if psd is not None:
        err = np.abs(np.asarray(psd, dtype=np.float64) - want["psd"]).max()
        assert err <= tol, ("psd", err, tol)
        worst = err / tol if tol > 0 else 0.0
    for b in range(4):
        nb = int((g["band"] == b).sum()) if b < 3 else g["F"]
        t = nb * tol + nb * EPS * abs(ws[5 + b])
        err = abs(float(stats[5 + b]) - ws[5 + b])
        assert err <= t, (STATS[5 + b], stats[5 + b], ws[5 + b], t)
        worst = max(worst, err / t) if t > 0 else worst
    q = np.float64(stats[6]) / np.float64(stats[7]) if stats[7] != 0 else (np.nan if stats[6] == 0 or np.isnan(stats[6]) else np.inf)
    if np.isnan(q):
        assert np.isnan(stats[9]), stats[9]
    elif np.isinf(q):
        assert stats[9] == q
    else:
        assert abs(float(stats[9]) - q) <= 2 * EPS * abs(q), ("lf_hf", stats[9], q)
    return float(worst)
