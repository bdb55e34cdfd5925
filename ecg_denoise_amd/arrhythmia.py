"""Rhythm findings on the device, window by window: atrial fibrillation (AF), tachy- and bradycardia, pauses and ventricular runs.

    fid = BeatDelineator(fs).delineate(records, beats); pst = PStMeasurer(fs).measure(records, fid)
    rh = ArrhythmiaAnalyzer(fs=360).analyse(beats, T, classes, pst)    # whole records, ral_arrhythmia_windows -> ArrhythmiaWindows
    rh.af, rh.nrmssd, rh.p_share, rh.episodes("af")                     # flags, evidence, (start, end) sample ranges per record
    ev = evaluate_af(denoiser, records, noise, snr_db, truth)           # the noise-stress protocol: is the rhythm diagnosis back?

The AF rule is "irregular RR and no P wave locked to the QRS".  RR irregularity alone cannot tell AF from frequent premature
beats, and "no P wave found" fails once fibrillatory waves are present - `PStMeasurer` accepts a peak of the f wave in most
beats - but the distance from that peak to the QRS onset is random in AF and constant in sinus rhythm: the P evidence is a
PR-consistency count, not a P-found count.

The definition (include/ralenet.h has the same one).  Input per record: strictly ascending beat positions p_0 < ... < p_{n-1} in
[0, T) - a `Beats`, or per-record lists; optionally labels l_i (a `BeatClasses`, or per-record lists), without them every beat is
N; optionally the P input on_i and ppeak_i, the fields of a `PStPoints`.  Geometry (`arrhythmia_geometry`; exact rational
arithmetic, round = nearest, halves up, fs an int or a Fraction; the values at 360 Hz):

    W = round(win_s fs) = 10800, H = round(hop_s fs) = 3600     window and hop (30 s, 10 s)
    lo_n = ceil(0.3 fs) = 108, hi_n = floor(2.0 fs) = 720       the accepted intervals
    bin = max(1, round(fs / 40)) = 9 (25 ms), G = 24            the Lorenz grid is (2G + 1)^2 cells
    lock_n = round(fs / 50) = 7 (20 ms), prmax = round(0.4 fs) = 144
    pause_n = floor(pause_s fs) = 720 (pause_s = 2.0), min_m = 12, vrun_min = 3, max_m = (W - 1) // lo_n = 99

The fp32 limits: n0 = 0.10, c0 = 0.6, pl0 = 0.5, tachy = 100, brady = 50.  Windows follow `hrv_windows`:
nw = max(1, (T - W) // H + 1), window w = [w H, min(w H + W, T)).  Per window [w0, w1):

    members       beat i is a member iff w0 <= p_i < w1.  beats = their number; nv = the members with label 1; vrun = the longest
                  run of consecutive list indices that are all members with label 1; pauses = #{i >= 1: p_{i-1} and p_i members
                  and d_i = p_i - p_{i-1} > pause_n}, whatever the labels
    accepted      interval i >= 1 is accepted iff both beats are members, neither has label 1 and lo_n <= d_i <= hi_n (labels 2 and
                  -1 stay in: AF beats look premature to the classifier).  m = their number, S1 = sum d (64 bits)
    differences   D_i = d_i - d_{i-1} where intervals i - 1 and i are both accepted.  k = their number, D2 = sum D^2 (64 bits)
    Lorenz        a point is a pair (D_{i-1}, D_i) with both defined; k2 = the number of points;
                  cell(D) = clamp(floor((2 D + bin) / (2 bin)), -G, G), floor towards minus infinity; nec = the number of
                  distinct cells that hold a point; origin = the number of points in cell (0, 0)
    P evidence    only with the P input, otherwise p_meas = p_found = p_locked = 0 and pr_med = -1.  A measured beat is a member
                  with label != 1 and on_i >= 0: p_meas.  It is found iff ppeak_i >= 0 and 1 <= on_i - ppeak_i <= prmax (the
                  difference in 64 bits): p_found, pr_i = that difference.  pr_med = the lower median sorted[(n - 1) // 2] of
                  the pr_i, -1 if there are none; p_locked = #{|pr_i - pr_med| <= lock_n}
    stats         fp32, each computed in fp64 from the exact integers and rounded once, NaN where its denominator is missing:
                  mean_rr = S1 / (m fs), hr = 60 m fs / S1 (m >= 1); nrmssd = sqrt(D2 / k) / (S1 / m) (k >= 1);
                  nec_ratio = nec / k2 (k2 >= 1); p_share = p_locked / p_meas (p_meas >= 1)
    flags         int32, each bit decided on the device from the returned fp32 values against the fp32 limits:
                  32 IRREGULAR  m >= min_m and k2 >= 1 and nrmssd >= n0 and nec_ratio >= c0
                   1 AF         IRREGULAR and not (p_share >= pl0): a NaN p_share (no P input, nothing measurable) passes
                   2 TACHY      m >= 1 and hr > tachy             4 BRADY   m >= 1 and hr < brady
                   8 PAUSE      pauses >= 1                      16 VRUN    vrun >= vrun_min

Output per window: counts (13) int32 = [beats, m, k, k2, nec, origin, p_meas, p_found, p_locked, pr_med, pauses, nv, vrun];
stats (5) fp32 = [mean_rr, hr, nrmssd, nec_ratio, p_share]; flags int32.  Every count is an exact integer and there is no
floating-point sum, so the results equal a numpy restatement bit for bit.  Supported (`arrhythmia_check`): 2 <= W < 2^31, 1 <= H,
1 <= lo_n <= hi_n, max_m <= 4096, 1 <= bin, 1 <= G <= 64, 0 <= lock_n, 1 <= prmax <= 8192, 1 <= pause_n, 2 <= min_m,
1 <= vrun_min, finite limits.

The defaults were chosen on synthetic data (`synth`) only; none has been tuned on a database.

Device tensors only: there is no CPU fallback."""
import numbers

import numpy as np
import torch

from . import _lib
from .beats import MODEL_RATE, BeatDetector, _round
from .delineate import BeatDelineator
from .evaluate import stress_front
from .hrv import _labels, _sec, hrv_windows
from .intake import beat_lists
from .model import _ptr, _stream
from .pools import table_buffer
from .pst import PStMeasurer, PStPoints
from .rate import _rate
from .rhythm import BeatClassifier

COUNTS = ("beats", "m", "k", "k2", "nec", "origin", "p_meas", "p_found", "p_locked", "pr_med", "pauses", "nv", "vrun")
STATS = ("mean_rr", "hr", "nrmssd", "nec_ratio", "p_share")
FLAGS = {"af": 1, "tachy": 2, "brady": 4, "pause": 8, "vrun": 16, "irregular": 32}
_LIMITS = ("n0", "c0", "pl0", "tachy", "brady")
_MAX_M, _MAX_G, _MAX_PR = 4096, 64, 8192


def arrhythmia_geometry(fs=MODEL_RATE, win_s=30, hop_s=10, n0=0.10, c0=0.6, pl0=0.5, tachy=100, brady=50, pause_s=2.0, min_m=12):
    """-> {fs, W, H, lo_n, hi_n, bin, G, lock_n, prmax, pause_n, min_m, vrun_min, max_m, n0, c0, pl0, tachy, brady}: lengths in
    samples at rate `fs` (a positive int or Fraction), the limits as floats; nothing is refused here (`arrhythmia_check`)"""
    fs = _rate(fs, "fs")
    win, hop, pause = _sec(win_s, "win_s"), _sec(hop_s, "hop_s"), _sec(pause_s, "pause_s")
    if isinstance(min_m, bool) or not isinstance(min_m, numbers.Integral):
        raise _lib.RalError(f"arrhythmia: min_m must be an int (got {min_m!r})")
    g = {"fs": fs, "W": _round(win * fs), "H": _round(hop * fs), "lo_n": int(-((-fs * 3 / 10).__floor__())),
         "hi_n": int((2 * fs).__floor__()), "bin": max(1, _round(fs / 40)), "G": 24, "lock_n": _round(fs / 50),
         "prmax": _round(fs * 2 / 5), "pause_n": int((pause * fs).__floor__()), "min_m": int(min_m), "vrun_min": 3}
    g["max_m"] = (g["W"] - 1) // g["lo_n"] if g["lo_n"] >= 1 else 0
    for name, v in zip(_LIMITS, (n0, c0, pl0, tachy, brady)):
        if isinstance(v, bool) or not isinstance(v, (numbers.Real, np.floating)):
            raise _lib.RalError(f"arrhythmia: {name} must be a number (got {v!r})")
        g[name] = float(v)
    return g


def arrhythmia_check(g):
    """raise RalError, naming the broken rule, unless the geometry is one ral_arrhythmia_windows supports -> the geometry"""
    rules = (("2 <= W < 2^31", 2 <= g["W"] < 2 ** 31), ("1 <= H", 1 <= g["H"]), ("1 <= lo_n <= hi_n", 1 <= g["lo_n"] <= g["hi_n"]),
             ("max_m = (W - 1) // lo_n <= 4096", g["max_m"] <= _MAX_M), ("1 <= bin", 1 <= g["bin"]),
             ("1 <= G <= 64", 1 <= g["G"] <= _MAX_G), ("0 <= lock_n", 0 <= g["lock_n"]),
             ("1 <= prmax <= 8192", 1 <= g["prmax"] <= _MAX_PR), ("1 <= pause_n", 1 <= g["pause_n"]),
             ("2 <= min_m", 2 <= g["min_m"]), ("1 <= vrun_min", 1 <= g["vrun_min"]),
             ("finite limits n0, c0, pl0, tachy, brady", all(np.isfinite(np.float32(g[k])) for k in _LIMITS)))
    for rule, ok in rules:
        if not ok:
            raise _lib.RalError("arrhythmia: this geometry is not supported: need " + rule + " ("
                                + " ".join(f"{k}={g[k]}" for k in ("W", "H", "lo_n", "hi_n", "bin", "G", "lock_n", "prmax", "pause_n",
                                                                    "min_m", "vrun_min", "max_m") + _LIMITS) + f" at fs={g['fs']})")
    return g


def _runs(flagged, win):
    """flagged (nw,) bool and win (nw, 2) of one record -> [(w0 of the first, w1 of the last window) of every maximal run]"""
    out, start = [], None
    for w, f in enumerate(list(flagged) + [False]):
        if f and start is None:
            start = w
        elif not f and start is not None:
            out.append((int(win[start, 0]), int(win[w - 1, 1])))
            start = None
    return out


class ArrhythmiaWindows:
    """What `ArrhythmiaAnalyzer.analyse` returns, N windows record by record: `counts` (N, 13) int32 [beats, m, k, k2, nec,
    origin, p_meas, p_found, p_locked, pr_med, pauses, nv, vrun], `stats` (N, 5) fp32 [mean_rr, hr, nrmssd, nec_ratio, p_share]
    (seconds, beats per minute, ratios) and `flags` (N,) int32, all on the device; `index` (N, 2) int64 on the host, the record
    and the window's number, and `windows` (N, 2) int64 on the host, [w0, w1) in samples.  Every count and statistic is a view
    by its name (`nrmssd`, `nec`, `p_locked`, ...); `af`, `tachy`, `brady`, `pause`, `vrun` and `irregular` are bool tensors of
    the flag bits (`flag(kind)` gives them too), so the count of the longest ventricular run is `vrun_len`."""

    def __init__(self, counts, stats, flags, index, windows, geometry):
        self.counts, self.stats, self.flags, self.index, self.windows, self.geometry = counts, stats, flags, index, windows, geometry

    def __len__(self):
        return self.counts.shape[0]

    def flag(self, kind):
        """-> (N,) bool on the device: the bit `kind` (af, tachy, brady, pause, vrun, irregular)"""
        if kind not in FLAGS:
            raise _lib.RalError(f"ArrhythmiaWindows: no finding named {kind!r} (there are {', '.join(FLAGS)})")
        return (self.flags & FLAGS[kind]) != 0

    def __getattr__(self, name):
        if name in FLAGS:
            return self.flag(name)
        if name in STATS:
            return self.stats[:, STATS.index(name)]
        if name in COUNTS or name == "vrun_len":
            return self.counts[:, COUNTS.index("vrun" if name == "vrun_len" else name)]
        raise AttributeError(name)

    def tolist(self):
        """-> one dict per window: record, window, w0, w1, the 13 counts, the five statistics and flags (synchronises)"""
        keys = ("record", "window", "w0", "w1") + COUNTS + STATS + ("flags",)
        return [dict(zip(keys, tuple(ix) + tuple(w) + tuple(c) + tuple(s) + (f,)))
                for ix, w, c, s, f in zip(self.index.tolist(), self.windows.tolist(), self.counts.tolist(), self.stats.tolist(),
                                          self.flags.tolist())]

    def episodes(self, kind="af"):
        """-> per record the list of (start, end) sample ranges of the maximal runs of consecutive windows with the bit `kind`:
        start is w0 of the first window and end is w1 of the last (on the host; synchronises)"""
        hit = self.flag(kind).cpu().numpy()
        R = int(self.index[:, 0].max()) + 1 if len(self.index) else 0
        return [_runs(hit[self.index[:, 0] == r], self.windows[self.index[:, 0] == r]) for r in range(R)]


def _p_input(pst, pos, what):
    """`PStPoints` or None -> (on, ppeak) (R, cap) int32 on the device of `pos`, or (None, None)"""
    if pst is None:
        return None, None
    if not isinstance(pst, PStPoints):
        raise _lib.RalError(f"{what}: expected the PStPoints of PStMeasurer.measure, got {type(pst).__name__}")
    for name, t in (("on", pst.on), ("ppeak", pst.ppeak)):
        if t.shape != pos.shape or t.dtype != torch.int32 or t.device != pos.device:
            raise _lib.RalError(f"{what}: P input whose `{name}` is {tuple(t.shape)} {t.dtype} on {t.device} for positions "
                                f"{tuple(pos.shape)} {pos.dtype} on {pos.device}")
    return pst.on.contiguous(), pst.ppeak.contiguous()


class ArrhythmiaAnalyzer:
    """Rhythm findings of whole records at rate `fs` (`ral_arrhythmia_windows`).  `analyse(beats, T, classes=None, pst=None)` takes
    the beats of R records of T samples - a `Beats`, which is trusted, or per-record lists of strictly ascending positions in
    [0, T), which are checked on the host - their labels - a `BeatClasses`, per-record lists, or None: every beat is N - and
    their P input - the `PStPoints` of `PStMeasurer.measure` at these beats, or None: no P evidence, AF is then IRREGULAR - and
    returns the `ArrhythmiaWindows` of all records, record by record, window by window.  The defaults were chosen on synthetic
    data only and have not been tuned on a database."""

    def __init__(self, fs=MODEL_RATE, win_s=30, hop_s=10, n0=0.10, c0=0.6, pl0=0.5, tachy=100, brady=50, pause_s=2.0, min_m=12,
                 device="cuda"):
        self.fs = fs
        self.geometry = g = arrhythmia_check(arrhythmia_geometry(fs, win_s, hop_s, n0, c0, pl0, tachy, brady, pause_s, min_m))
        self.geom = _lib.ArrhythmiaGeom(g["W"], g["lo_n"], g["hi_n"], g["bin"], g["G"], g["lock_n"], g["prmax"], g["pause_n"],
                                        g["min_m"], g["vrun_min"], g["n0"], g["c0"], g["pl0"], g["tachy"], g["brady"], 0,
                                        float(g["fs"]))
        self.device = torch.device(device)

    @torch.no_grad()
    def analyse(self, beats, T, classes=None, pst=None):
        what = "ArrhythmiaAnalyzer.analyse"
        if isinstance(T, bool) or not isinstance(T, numbers.Integral) or not 1 <= T < 2 ** 31:
            raise _lib.RalError(f"{what}: T must be in [1, 2^31) (got {T!r})")
        pos, count = beat_lists(beats, self.device, what, T=int(T))
        label = _labels(classes, pos, count, what)
        on, ppeak = _p_input(pst, pos, what)
        if pos.device.type != "cuda":
            raise _lib.RalError(f"{what} runs on the GPU (there is no CPU fallback)")
        R, cap = pos.shape
        win = hrv_windows(T, self.geometry)
        nw = len(win)
        N = R * nw
        tab = np.zeros(N, dtype=_lib.HRV_ROW)
        tab["rec"], tab["w0"], tab["w1"] = np.repeat(np.arange(R), nw), np.tile(win[:, 0], R), np.tile(win[:, 1], R)
        index = np.stack([np.repeat(np.arange(R, dtype=np.int64), nw), np.tile(np.arange(nw, dtype=np.int64), R)], axis=1)
        dev = pos.device
        with torch.cuda.device(dev):
            counts = torch.empty(N, len(COUNTS), dtype=torch.int32, device=dev)
            stats = torch.empty(N, len(STATS), dtype=torch.float32, device=dev)
            flags = torch.empty(N, dtype=torch.int32, device=dev)
            tab_dev = table_buffer(tab, dev)
            opt = lambda t: None if t is None else _ptr(t)
            _lib.check(_lib.lib().ral_arrhythmia_windows(_ptr(pos), opt(label), _ptr(count), opt(on), opt(ppeak), R, cap,
                                                         tab.ctypes.data, N, _ptr(tab_dev), 1, self.geom, _ptr(counts),
                                                         _ptr(stats), _ptr(flags), _stream()))
        return ArrhythmiaWindows(counts, stats, flags, index, np.tile(win, (R, 1)), self.geometry)


class AfEvaluation:
    """What `evaluate_af` returns: `clean`, `noisy`, `denoised`, the `ArrhythmiaWindows` of the three records (the same windows in
    the same order); `scores` = {"clean": {tp, fp, fn, tn, sensitivity, specificity}, "noisy": {...}, "denoised": {...}}, the AF
    bit per window against `positive` over the windows `scored` (both (N,) bool on the host; sensitivity and specificity are NaN
    where their denominator is 0)."""

    def __init__(self, clean, noisy, denoised, scores, positive, scored):
        self.clean, self.noisy, self.denoised, self.scores, self.positive, self.scored = clean, noisy, denoised, scores, positive, scored


def af_truth(windows, index, truth):
    """windows (N, 2), index (N, 2) and per-record episode ranges [(start, end), ...] -> (positive, scored), (N,) bool: a window
    is positive when it lies wholly inside an episode, negative when it is disjoint from all of them, and left out otherwise"""
    pos, scored = np.zeros(len(windows), dtype=bool), np.zeros(len(windows), dtype=bool)
    for i, ((w0, w1), (r, _)) in enumerate(zip(windows.tolist(), index.tolist())):
        eps = [(int(s), int(e)) for s, e in truth[r]]
        inside = any(s <= w0 and w1 <= e for s, e in eps)
        apart = all(w1 <= s or e <= w0 for s, e in eps)
        pos[i], scored[i] = inside, inside or apart
    return pos, scored


def af_scores(flagged, positive, scored):
    """three (N,) bool arrays -> {tp, fp, fn, tn, sensitivity, specificity} over the scored windows"""
    f, p, s = (np.asarray(v, dtype=bool) for v in (flagged, positive, scored))
    tp, fp, fn, tn = (int((a & b & s).sum()) for a, b in ((f, p), (f, ~p), (~f, p), (~f, ~p)))
    return {"tp": tp, "fp": fp, "fn": fn, "tn": tn, "sensitivity": tp / (tp + fn) if tp + fn else float("nan"),
            "specificity": tn / (tn + fp) if tn + fp else float("nan")}


def evaluate_af(denoiser, records, noise, snr_db, truth=None, offsets=None, rng=None, detector=None, classifier=None,
                delineator=None, measurer=None, analyzer=None):
    """The noise-stress protocol scored in the rhythm diagnosis: `mix_records(records, noise, snr_db, offsets, rng)`,
    `denoiser.denoise(noisy)`, then the clean, the noisy and the denoised records EACH go detect -> classify -> delineate -> P/ST
    -> analyse on their own, as in `evaluate_hrv`: the beat positions and the P waves are what the noise damages.  Per condition
    the AF bit of every window is scored: without `truth` against the clean record's own flags over all windows; with `truth`
    (per record a list of (start, end) episode ranges in samples) a window is positive when it lies wholly inside an episode,
    negative when it is disjoint from all of them, and left out otherwise -> `AfEvaluation`.  detector, classifier, delineator,
    measurer and analyzer (defaults `BeatDetector(fs)`, `BeatClassifier(fs)`, `BeatDelineator(fs)`, `PStMeasurer(fs)`,
    `ArrhythmiaAnalyzer(fs)`) run at the denoiser's outer rate `fs`, 360 Hz where it names none."""
    fs, dev, clean, noisy, out = stress_front(denoiser, records, noise, snr_db, offsets, rng)
    det, cls = detector or BeatDetector(fs, device=dev), classifier or BeatClassifier(fs, device=dev)
    dl, ms = delineator or BeatDelineator(fs, device=dev), measurer or PStMeasurer(fs, device=dev)
    ana = analyzer or ArrhythmiaAnalyzer(fs, device=dev)
    if truth is not None and len(truth) != clean.shape[0]:
        raise _lib.RalError(f"evaluate_af: truth for {len(truth)} records, {clean.shape[0]} records given")
    res = []
    for x in (clean, noisy, out):
        beats = det.detect(x)
        res.append(ana.analyse(beats, x.shape[-1], cls.classify(x, beats), ms.measure(x, dl.delineate(x, beats))))
    flagged = [r.af.cpu().numpy() for r in res]
    if truth is None:
        positive, scored = flagged[0].copy(), np.ones(len(flagged[0]), dtype=bool)
    else:
        positive, scored = af_truth(res[0].windows, res[0].index, truth)
    scores = {key: af_scores(f, positive, scored) for key, f in zip(("clean", "noisy", "denoised"), flagged)}
    return AfEvaluation(res[0], res[1], res[2], scores, positive, scored)
