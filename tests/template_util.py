"""The numpy oracle of the median beat (include/ralenet.h, "median beat"; ecg_denoise_amd/template.py): the definition stated
explicitly - the members of every window in list order, `np.sort` over the member axis, the middle value or
(a + b) * np.float32(0.5), the lower integer median for rr - and the comparison with the device.  The definition holds no
expression a compiler could contract into an FMA, so the comparison is exact equality of values (-0.0 == 0.0)."""
from fractions import Fraction

import numpy as np

KMAX = 256
F = np.float32


def _round(v):
    """nearest integer, halves up, in exact rational arithmetic"""
    return int((Fraction(v) + Fraction(1, 2)).__floor__())


def geometry(fs, win_s=10, hop_s=10):
    fs = Fraction(fs)
    pre, post = _round(fs * Fraction(35, 100)), _round(fs * Fraction(65, 100))
    return {"fs": fs, "Wpre": pre, "Wpost": post, "Wn": pre + post + 1, "W": _round(Fraction(win_s) * fs),
            "H": _round(Fraction(hop_s) * fs), "KMAX": KMAX}


def windows(T, g):
    """-> [(w0, w1)]: window w = [w H, min(w H + W, T)), nw = max(1, (T - W) // H + 1)"""
    return [(w * g["H"], min(w * g["H"] + g["W"], T)) for w in range(max(1, (T - g["W"]) // g["H"] + 1))]


def members(pos, labels, T, w0, w1, g):
    """-> the list indices of the members of the window [w0, w1), in list order"""
    return [i for i, p in enumerate(pos) if w0 <= p < w1 and (labels is None or labels[i] == 0)
            and p - g["Wpre"] >= 0 and p + g["Wpost"] <= T - 1]


def median_beats(x, pos, labels, g):
    """x (leads, T) np.float32, pos the record's beats, labels one per beat or None -> {"template" (nw, leads, Wn) float32,
    "used", "total", "rr" (nw,) int32}"""
    assert x.dtype == np.float32
    leads, T = x.shape
    pos = [int(p) for p in pos]
    win = windows(T, g)
    out = {"template": np.zeros((len(win), leads, g["Wn"]), dtype=F), "used": np.zeros(len(win), dtype=np.int32),
           "total": np.zeros(len(win), dtype=np.int32), "rr": np.full(len(win), -1, dtype=np.int32)}
    for w, (w0, w1) in enumerate(win):
        mem = members(pos, labels, T, w0, w1, g)
        use = mem[:g["KMAX"]]
        out["total"][w], out["used"][w] = len(mem), len(use)
        if use:
            stack = np.stack([x[:, pos[i] - g["Wpre"]:pos[i] + g["Wpost"] + 1] for i in use])       # (used, leads, Wn)
            s = np.sort(stack, axis=0)
            n = len(use)
            out["template"][w] = s[n // 2] if n % 2 else F(s[n // 2 - 1] + s[n // 2]) * F(0.5)
        d = sorted(pos[i] - pos[i - 1] for i in use if i >= 1)
        if d:
            out["rr"][w] = d[(len(d) - 1) // 2]
    return out


def median_beats_records(x, lists, labels, g):
    """x (R, leads, T) -> the same dict with a leading record axis"""
    rows = [median_beats(np.ascontiguousarray(x[r], dtype=F), lists[r], None if labels is None else labels[r], g)
            for r in range(len(lists))]
    return {k: np.stack([row[k] for row in rows]) for k in rows[0]}


def compare(got, want):
    """got: a `BeatTemplates` (or a dict of arrays); want: the oracle's dict.  Asserts np.array_equal for template, used, total
    and rr (array_equal compares values: -0.0 == 0.0)"""
    for k in ("used", "total", "rr", "template"):
        a = got[k] if isinstance(got, dict) else getattr(got, k)
        a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
        assert a.shape == want[k].shape and a.dtype == want[k].dtype, (k, a.shape, a.dtype, want[k].shape, want[k].dtype)
        if not np.array_equal(a, want[k]):
            bad = np.argwhere(a != want[k])
            raise AssertionError(f"{k}: {len(bad)} of {a.size} values differ, first at {tuple(bad[0])}: device "
                                 f"{a[tuple(bad[0])]!r}, oracle {want[k][tuple(bad[0])]!r}")
