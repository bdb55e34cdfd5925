"""The numpy oracle of the rhythm findings (include/ralenet.h, "rhythm findings"; ecg_denoise_amd/arrhythmia.py): a restatement
of the definition one window at a time and one beat at a time, in Python integers, with every statistic formed in np.float64 and
rounded once to np.float32, and the comparison with the device.  Every count is an exact integer and no floating-point sum is
taken, so the comparison is exact equality of the 13 counts and of the flags and bit equality of the five statistics, NaN
positions included: no tolerance, no exemption."""
import math
from fractions import Fraction

import numpy as np

COUNTS = ("beats", "m", "k", "k2", "nec", "origin", "p_meas", "p_found", "p_locked", "pr_med", "pauses", "nv", "vrun")
STATS = ("mean_rr", "hr", "nrmssd", "nec_ratio", "p_share")
AF, TACHY, BRADY, PAUSE, VRUN, IRREGULAR = 1, 2, 4, 8, 16, 32
F = np.float32


def _round(q):
    """nearest, halves up, of a Fraction"""
    return int(math.floor(q + Fraction(1, 2)))


def geometry(fs=360, win_s=30, hop_s=10, pause_s=2.0, min_m=12, n0=0.10, c0=0.6, pl0=0.5, tachy=100, brady=50):
    fs = Fraction(fs)
    win, hop, pause = (Fraction(repr(v)) if isinstance(v, float) else Fraction(v) for v in (win_s, hop_s, pause_s))
    W, lo_n = _round(win * fs), int(math.ceil(Fraction(3, 10) * fs))
    return {"fs": fs, "W": W, "H": _round(hop * fs), "lo_n": lo_n, "hi_n": int(math.floor(2 * fs)), "bin": max(1, _round(fs / 40)),
            "G": 24, "lock_n": _round(fs / 50), "prmax": _round(Fraction(2, 5) * fs), "pause_n": int(math.floor(pause * fs)),
            "min_m": min_m, "vrun_min": 3, "max_m": (W - 1) // lo_n,
            "n0": F(n0), "c0": F(c0), "pl0": F(pl0), "tachy": F(tachy), "brady": F(brady)}


def windows(T, g):
    nw = max(1, (T - g["W"]) // g["H"] + 1)
    return [(w * g["H"], min(w * g["H"] + g["W"], T)) for w in range(nw)]


def cell(D, g):
    return min(max((2 * D + g["bin"]) // (2 * g["bin"]), -g["G"]), g["G"])          # (Python's // floors towards minus infinity)


def window(pos, lab, on, ppeak, w0, w1, g):
    """one window [w0, w1) of one record: pos the ascending positions, lab the labels or None, on and ppeak the P input or None
    (both) -> (13 ints, (5,) np.float32, flags)"""
    n = len(pos)
    pos = [int(p) for p in pos]
    lab = [0] * n if lab is None else [int(l) for l in lab]
    member = [w0 <= p < w1 for p in pos]
    beats = sum(member)
    nv = sum(1 for i in range(n) if member[i] and lab[i] == 1)
    vrun = run = 0
    for i in range(n):
        run = run + 1 if member[i] and lab[i] == 1 else 0
        vrun = max(vrun, run)
    d = [None] + [pos[i] - pos[i - 1] for i in range(1, n)]
    both = [False] + [member[i - 1] and member[i] for i in range(1, n)]
    pauses = sum(1 for i in range(1, n) if both[i] and d[i] > g["pause_n"])
    acc = [False] + [both[i] and lab[i] != 1 and lab[i - 1] != 1 and g["lo_n"] <= d[i] <= g["hi_n"] for i in range(1, n)]
    m = sum(acc)
    S1 = sum(d[i] for i in range(1, n) if acc[i])
    D = {i: d[i] - d[i - 1] for i in range(2, n) if acc[i] and acc[i - 1]}
    k = len(D)
    D2 = sum(v * v for v in D.values())
    points = [(cell(D[i - 1], g), cell(D[i], g)) for i in D if i - 1 in D]
    k2, nec, origin = len(points), len(set(points)), sum(1 for c in points if c == (0, 0))
    p_meas = p_found = p_locked = 0
    pr_med = -1
    if on is not None:
        pr = []
        for i in range(n):
            if member[i] and lab[i] != 1 and int(on[i]) >= 0:
                p_meas += 1
                diff = int(on[i]) - int(ppeak[i])
                if int(ppeak[i]) >= 0 and 1 <= diff <= g["prmax"]:
                    pr.append(diff)
        p_found = len(pr)
        if pr:
            pr_med = sorted(pr)[(len(pr) - 1) // 2]
            p_locked = sum(1 for v in pr if abs(v - pr_med) <= g["lock_n"])
    fs = np.float64(float(g["fs"]))
    nan = F(np.nan)
    dm, dS1 = np.float64(m), np.float64(S1)
    mean_rr = F(dS1 / (dm * fs)) if m >= 1 else nan
    hr = F(np.float64(60.0) * dm * fs / dS1) if m >= 1 else nan
    nrmssd = F(np.sqrt(np.float64(D2) / np.float64(k)) / (dS1 / dm)) if k >= 1 else nan
    nec_ratio = F(np.float64(nec) / np.float64(k2)) if k2 >= 1 else nan
    p_share = F(np.float64(p_locked) / np.float64(p_meas)) if p_meas >= 1 else nan
    irregular = m >= g["min_m"] and k2 >= 1 and bool(nrmssd >= g["n0"]) and bool(nec_ratio >= g["c0"])
    flags = 0
    if irregular:
        flags |= IRREGULAR
        if not bool(p_share >= g["pl0"]):
            flags |= AF
    if m >= 1 and bool(hr > g["tachy"]):
        flags |= TACHY
    if m >= 1 and bool(hr < g["brady"]):
        flags |= BRADY
    if pauses >= 1:
        flags |= PAUSE
    if vrun >= g["vrun_min"]:
        flags |= VRUN
    counts = (beats, m, k, k2, nec, origin, p_meas, p_found, p_locked, pr_med, pauses, nv, vrun)
    return counts, np.array([mean_rr, hr, nrmssd, nec_ratio, p_share], dtype=np.float32), flags


def analyse(beats, T, g, labels=None, on=None, ppeak=None):
    """per-record lists -> (counts (N, 13) int64, stats (N, 5) float32, flags (N,) int64, index (N, 2) int64), record by record,
    window by window"""
    counts, stats, flags, index = [], [], [], []
    for r, pos in enumerate(beats):
        for w, (w0, w1) in enumerate(windows(T, g)):
            c, s, f = window(pos, None if labels is None else labels[r], None if on is None else on[r],
                             None if ppeak is None else ppeak[r], w0, w1, g)
            counts.append(c), stats.append(s), flags.append(f), index.append((r, w))
    return (np.array(counts, dtype=np.int64).reshape(-1, 13), np.array(stats, dtype=np.float32).reshape(-1, 5),
            np.array(flags, dtype=np.int64), np.array(index, dtype=np.int64).reshape(-1, 2))


def same_bits(a, b):
    """two float32 arrays: equal shapes, NaN in the same places, and the same bits everywhere else"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint32), b[ok].view(np.uint32))


def compare(got, want):
    """got: an ArrhythmiaWindows (or a (counts, stats, flags) triple of arrays); want: what `analyse` returned.  Asserts exact
    equality row by row, naming the first row and field that differs."""
    if hasattr(got, "counts"):
        got = (got.counts.cpu().numpy(), got.stats.cpu().numpy(), got.flags.cpu().numpy())
    gc, gs, gf = (np.asarray(v) for v in got)
    wc, ws, wf = want[:3]
    assert gc.shape == wc.shape and gs.shape == ws.shape and gf.shape == wf.shape, (gc.shape, wc.shape, gs.shape, gf.shape)
    for r in range(len(wc)):
        assert tuple(int(v) for v in gc[r]) == tuple(int(v) for v in wc[r]), \
            f"row {r}: counts device {dict(zip(COUNTS, gc[r].tolist()))}, oracle {dict(zip(COUNTS, wc[r].tolist()))}"
        assert same_bits(gs[r], ws[r]), f"row {r}: stats device {gs[r]}, oracle {ws[r]} (counts {wc[r].tolist()})"
        assert int(gf[r]) == int(wf[r]), f"row {r}: flags device {int(gf[r])}, oracle {int(wf[r])} (stats {ws[r]})"
