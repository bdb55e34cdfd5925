"""The numpy oracle of the P-wave and ST-level measurement (include/ralenet.h, "P wave and ST level";
ecg_denoise_amd/pst.py): a restatement of the definition one beat at a time and one sample at a time, in np.float32 with every sum
in the stated order, and the comparison with the device.  The definition holds no expression a compiler could contract into an
FMA, so the comparison is exact equality of the three integers of every beat and bit equality of its ST levels, NaN positions
included: no tolerance, no exemption."""
from fractions import Fraction

import numpy as np

from delineate_util import _round, delineate_record

P0 = 0.08
F = np.float32


def geometry(fs):
    fs = Fraction(fs)
    return {"m2": _round(fs / 60), "g": _round(fs / 50), "Wp": _round(fs * Fraction(30, 100)), "j": _round(fs * Fraction(6, 100))}


def scale(fs):
    """w: the fp64 quotient 1 / (2 m2 + 1), rounded once"""
    return F(1.0 / (2 * geometry(fs)["m2"] + 1))


def measure_beat(x, p, on, off, prev=None, nxt=None, fs=360, p0=P0):
    """the beat at p of the record x (leads, T), np.float32, with the delineator's on and off; prev, nxt: the neighbouring
    beats' positions or None -> (pon, ppeak, poff, st): three ints and a (leads,) np.float32 array"""
    assert x.dtype == np.float32
    G = geometry(fs)
    m2, g, Wp, j = (G[k] for k in ("m2", "g", "Wp", "j"))
    w = scale(fs)
    leads, T = x.shape
    p, on, off = int(p), int(on), int(off)
    nan = np.full(leads, np.nan, dtype=np.float32)
    has_on, has_off = 0 <= on <= p, p <= off <= T - 1
    if not has_on:
        return -1, -1, -1, nan

    def c(t):
        return min(max(t, 0), T - 1)

    z_seen, s_seen = {}, {}

    def z(l, t):
        if (l, t) not in z_seen:
            acc = F(0)
            for k in range(-m2, m2 + 1):
                acc = F(acc + x[l, c(t + k)])
            z_seen[l, t] = acc
        return z_seen[l, t]

    e = max(on - g, 0)
    b = [z(l, e) for l in range(leads)]

    def s(t):
        if t not in s_seen:
            acc = F(0)
            for l in range(leads):
                acc = F(acc + F(abs(F(z(l, t) - b[l]))))
            s_seen[t] = acc
        return s_seen[t]

    st = nan
    if has_off:
        ts, lim = off + j, T - 1
        if nxt is not None:
            lim = min(lim, p + (2 * (int(nxt) - p)) // 3)
        if ts <= lim:
            st = np.array([F(F(z(l, ts) - b[l]) * w) for l in range(leads)], dtype=np.float32)

    none = (-1, -1, -1, st)
    phi, plo = e, max(on - Wp, 0)
    if prev is not None:
        plo = max(plo, int(prev) + (2 * (p - int(prev))) // 3)
    if plo > phi:
        return none
    ppeak = plo
    for t in range(plo, phi + 1):
        if s(t) > s(ppeak):
            ppeak = t
    if ppeak == plo or ppeak == phi or s(ppeak) == 0:
        return none
    S = F(0)
    for t in range(on, max(off, p) + 1 if has_off else p + 1):
        S = max(S, s(t))
    if s(ppeak) < F(F(p0) * S):
        return none
    pon, best = plo, None
    for t in range(plo, ppeak + 1):
        area = F(F(s(ppeak) - s(t)) * F(t + ppeak - 2 * plo))
        if best is None or area > best:
            pon, best = t, area
    poff, best = ppeak, None
    for t in range(ppeak, phi + 1):
        area = F(F(s(ppeak) - s(t)) * F(2 * phi - ppeak - t))
        if best is None or area > best:
            poff, best = t, area
    return pon, ppeak, poff, st


def measure_record(x, pos, on, off, fs=360, p0=P0):
    """-> (pon, ppeak, poff, st): three lists of one int per beat and an (n, leads) np.float32 array"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = len(pos)
    out = [measure_beat(x, pos[i], on[i], off[i], pos[i - 1] if i else None, pos[i + 1] if i + 1 < n else None, fs, p0)
           for i in range(n)]
    st = np.stack([o[3] for o in out]) if n else np.zeros((0, x.shape[0]), np.float32)
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out], st


def delineate_and_measure(x, pos, fs=360, p0=P0, q0=0.15):
    """the delineator's oracle and then this one -> (on, off, pon, ppeak, poff, st)"""
    on, off, _, _ = delineate_record(x, pos, fs, q0)
    return (on, off) + measure_record(x, pos, on, off, fs, p0)


def same_bits(a, b):
    """two float32 arrays: equal shapes, NaN in the same places, and the same bits everywhere else"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint32), b[ok].view(np.uint32))


def compare(x, pos, on, off, got, fs=360, p0=P0):
    """x (leads, T), pos, the on and off the device was given, got = (pon, ppeak, poff lists, st (n, leads)) of the device for
    this record: asserts that the integers of every beat are the oracle's and that st has the oracle's bits -> the oracle's"""
    want = measure_record(x, pos, on, off, fs, p0)
    assert all(len(g) == len(pos) for g in got), ([len(g) for g in got], len(pos))
    for i in range(len(pos)):
        mine, theirs = tuple(int(g[i]) for g in got[:3]), tuple(w[i] for w in want[:3])
        assert mine == theirs, f"beat {i} of {len(pos)} at {pos[i]}: device {mine}, oracle {theirs}"
        assert same_bits(got[3][i], want[3][i]), f"beat {i} of {len(pos)} at {pos[i]}: st device {got[3][i]}, oracle {want[3][i]}"
    return want
