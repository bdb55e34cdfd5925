"""Heart rate and heart-rate variability (HRV) of classified beats on the device, window by window.

    hrv = HrvAnalyzer(fs=360).analyse(beats, T, classes)           # whole records, ral_hrv_windows -> HrvWindows
    pool = HrvPool(leads, capacity, fs=360)                        # chunks of independent streams: BeatClassPool + ral_hrv_windows
    ev = evaluate_hrv(denoiser, records, noise, snr_db)            # the noise-stress protocol scored in rhythm statistics

The definition (include/ralenet.h has the same one).  Input per record: an ascending list of beat positions p_0 < ... < p_{n-1}
in [0, T) - a `Beats`, or per-record lists - and optionally labels l_i (a `BeatClasses`, or per-record lists); without labels
every beat counts as N.  Geometry (`hrv_geometry`; exact rational arithmetic, round = nearest, halves up):

    W = round(win_s fs), H = round(hop_s fs)      window and hop in samples (300 s, 60 s)
    lo_n = ceil(nn_lo fs), hi_n = floor(nn_hi fs) the accepted intervals (0.3 s .. 2.0 s)
    t50 = floor(fs / 20)                          for an integer D: |D| > t50 iff |D| > 50 ms
    F = floor(fmax W / fs)                        frequency bins (fmax = 2/5 Hz), f_k = (k + 1) fs / W Hz for k = 0 .. F - 1
    band[k]                                       0 (VLF) if f_k < 0.04, 1 (LF) if 0.04 <= f_k < 0.15, 2 (HF) if 0.15 <= f_k < 0.4, else -1
    min_nn = 16                                   fewest NN intervals for a spectrum;  max_m = (W - 1) // lo_n

Windows of a record of length T: nw = max(1, (T - W) // H + 1), window w = [w H, min(w H + W, T)); a record shorter than W has the
single window [0, T); W stays the frequency base.  In a window, beats = #{w0 <= p_i < w1}; interval i >= 1, d_i = p_i - p_{i-1},
is NN iff w0 <= p_{i-1}, p_i < w1, l_{i-1} == 0 == l_i and lo_n <= d_i <= hi_n; the NN intervals in beat order are
(q_j = p_i - w0, d_j), j = 0 .. m - 1; a pair is two NN intervals of consecutive beat indices, D = d_i - d_{i-1}, k pairs,
n50 = #{|D| > t50}.  Time domain, from the exact integers S1 = sum d, S2 = sum d^2, D2 = sum D^2 in fp64, rounded once to fp32,
NaN where the denominator is missing:

    mean_nn = S1 / (m fs), hr = 60 m fs / S1 (m >= 1);  sdnn = sqrt((m S2 - S1^2) / (m (m - 1))) / fs (m >= 2);
    rmssd = sqrt(D2 / k) / fs, pnn50 = n50 / k (k >= 1)

Spectrum (m >= min_nn, else NaN): the Lomb-Scargle periodogram of y_j = fp32(d_j - S1 / m) at the phases 2 pi r / W with
r = ((k + 1) q_j) mod W exact; fp32 sums over j ascending YC, YS, CC, SS, CS; theta = atan2(2 CS, CC - SS) / 2; yc = ct YC + st YS,
ys = ct YS - st YC, cc = ct^2 CC + 2 ct st CS + st^2 SS, ss = ct^2 SS - 2 ct st CS + st^2 CC; P_k = (yc^2 / cc + ys^2 / ss) / 2 (a
term with denominator 0 counts as 0); psd_k = 2 P_k / (m fs^2) in s^2; vlf, lf, hf, total = the fp32 sums of psd_k over each band
and over all bins, ascending in k; lf_hf = lf / hf.

Output per window: counts [beats, m, k, n50] int32; stats [mean_nn, hr, sdnn, rmssd, pnn50, vlf, lf, hf, total, lf_hf] fp32;
optionally psd (F) fp32.  Supported (`hrv_check`): 2 <= W < 2^31, 1 <= H, 1 <= lo_n <= hi_n, 1 <= F <= 4096, F W < 2^31,
max_m <= 4096, 2 <= min_nn.

A window's values depend on the intervals relative to its origin alone and every floating-point sum has a fixed order, so a
stream analysed push by push (`HrvPool`) gives the bits of the complete record.

Device tensors only: there is no CPU fallback."""
import numbers
from fractions import Fraction

import numpy as np
import torch

from . import _lib
from .beats import MODEL_RATE, BeatDetector, _round
from .evaluate import stress_front
from .intake import beat_lists, pad_rows
from .model import _ptr, _stream
from .pools import StreamSurface, as_chunks, pack_chunks, table_buffer
from .rate import _rate
from .rhythm import BeatClasses, BeatClassifier, BeatClassPool

STATS = ("mean_nn", "hr", "sdnn", "rmssd", "pnn50", "vlf", "lf", "hf", "total", "lf_hf")
COUNTS = ("beats", "n_nn", "pairs", "n50")
_MAX_M = _MAX_F = 4096
_VLF_LF, _LF_HF, _HF_END = Fraction(1, 25), Fraction(3, 20), Fraction(2, 5)


def _sec(v, what):
    """seconds or hertz as an exact rational: an int, a Fraction, or a float read by its shortest decimal form"""
    if isinstance(v, bool) or not isinstance(v, (numbers.Integral, Fraction, float, np.floating)):
        raise _lib.RalError(f"hrv: {what} must be a number (got {v!r})")
    if isinstance(v, (float, np.floating)):
        if not np.isfinite(v):
            raise _lib.RalError(f"hrv: {what} must be finite (got {v!r})")
        return Fraction(repr(float(v)))
    return Fraction(v)


def hrv_geometry(fs=MODEL_RATE, win_s=300, hop_s=60, nn_range=(0.3, 2.0), fmax=Fraction(2, 5), min_nn=16):
    """-> {fs, W, H, lo_n, hi_n, t50, F, min_nn, max_m, band (F int32), freqs (F float64, Hz)} in samples at rate `fs` (a positive
    int or Fraction); nothing is refused here (`hrv_check`)"""
    fs = _rate(fs, "fs")
    win, hop, fmax = _sec(win_s, "win_s"), _sec(hop_s, "hop_s"), _sec(fmax, "fmax")
    lo, hi = (_sec(v, "nn_range") for v in nn_range)
    if isinstance(min_nn, bool) or not isinstance(min_nn, numbers.Integral):
        raise _lib.RalError(f"hrv: min_nn must be an int (got {min_nn!r})")
    W, H = _round(win * fs), _round(hop * fs)
    lo_n, hi_n = -((-lo * fs).__floor__()), (hi * fs).__floor__()
    F = (fmax * W / fs).__floor__() if W > 0 else 0
    nb = max(0, min(F, _MAX_F + 1))                  # (a refused F is not expanded into arrays)
    fk = [(k + 1) * fs / W for k in range(nb)]
    band = np.array([0 if f < _VLF_LF else 1 if f < _LF_HF else 2 if f < _HF_END else -1 for f in fk], dtype=np.int32)
    return {"fs": fs, "W": int(W), "H": int(H), "lo_n": int(lo_n), "hi_n": int(hi_n), "t50": int((fs / 20).__floor__()),
            "F": int(F), "min_nn": int(min_nn), "max_m": int((W - 1) // lo_n) if lo_n >= 1 else 0, "band": band,
            "freqs": np.array([float(f) for f in fk], dtype=np.float64)}


def hrv_check(g):
    """raise RalError, naming the broken rule, unless the geometry is one ral_hrv_windows supports -> the geometry"""
    rules = (("2 <= W < 2^31", 2 <= g["W"] < 2 ** 31), ("1 <= H", 1 <= g["H"]), ("1 <= lo_n <= hi_n", 1 <= g["lo_n"] <= g["hi_n"]),
             ("1 <= F <= 4096", 1 <= g["F"] <= _MAX_F), ("F * W < 2^31", g["F"] * g["W"] < 2 ** 31),
             ("max_m = (W - 1) // lo_n <= 4096", g["max_m"] <= _MAX_M), ("2 <= min_nn", 2 <= g["min_nn"]))
    for rule, ok in rules:
        if not ok:
            raise _lib.RalError(f"hrv: this geometry is not supported: need {rule} (W={g['W']} H={g['H']} lo_n={g['lo_n']} "
                                f"hi_n={g['hi_n']} F={g['F']} max_m={g['max_m']} min_nn={g['min_nn']} at fs={g['fs']})")
    return g


def hrv_windows(T, g):
    """the windows of a record of T samples -> (nw, 2) int64: [w0, w1) of window w = [w H, min(w H + W, T))"""
    T = int(T)
    if T < 1:
        raise _lib.RalError(f"hrv_windows: T must be >= 1 (got {T})")
    w0 = np.arange(max(1, (T - g["W"]) // g["H"] + 1), dtype=np.int64) * g["H"]
    return np.stack([w0, np.minimum(w0 + g["W"], T)], axis=1)


class HrvWindows:
    """What `HrvAnalyzer.analyse` and `HrvPool.push` return, N windows: `counts` (N, 4) int32 [beats, m, k, n50], `stats` (N, 10)
    fp32 [mean_nn, hr, sdnn, rmssd, pnn50, vlf, lf, hf, total, lf_hf] (seconds, beats per minute, s^2), `psd` (N, F) fp32 or
    None, all on the device, and `index` (N, 2) int64 on the host: the record (of a pool: the stream id) and the window's
    number.  Every statistic is a view by its name (`hr`, `sdnn`, ...), `n_nn` is m; `geometry` has `freqs` and `band`."""

    def __init__(self, counts, stats, psd, index, geometry):
        self.counts, self.stats, self.psd, self.index, self.geometry = counts, stats, psd, index, geometry

    def __len__(self):
        return self.counts.shape[0]

    def __getattr__(self, name):
        if name in STATS:
            return self.stats[:, STATS.index(name)]
        if name in COUNTS:
            return self.counts[:, COUNTS.index(name)]
        raise AttributeError(name)

    def tolist(self):
        """-> one dict per window: record, window, the four counts and the ten statistics as plain numbers (synchronises)"""
        return [dict(zip(("record", "window") + COUNTS + STATS, tuple(ix) + tuple(c) + tuple(s)))
                for ix, c, s in zip(self.index.tolist(), self.counts.tolist(), self.stats.tolist())]


class _Engine:
    """one geometry on one device: the C structure, the band array, the launch"""

    def __init__(self, geometry, device):
        self.geometry, g = hrv_check(geometry), geometry
        self.geom = _lib.HrvGeom(g["W"], g["lo_n"], g["hi_n"], g["t50"], g["F"], g["min_nn"], float(g["fs"]))
        self.device, self.band = torch.device(device), None

    def run(self, pos, label, count, rec, win, index, psd):
        """pos, count (and label or None) on the device; rec (N,), win (N, 2): the table -> HrvWindows"""
        dev, g, N = pos.device, self.geometry, len(rec)
        if dev.type != "cuda":
            raise _lib.RalError("hrv runs on the GPU (there is no CPU fallback)")
        if self.band is None or self.band.device != dev:
            self.band = torch.from_numpy(g["band"]).to(dev)
        tab = np.zeros(N, dtype=_lib.HRV_ROW)
        tab["rec"], tab["w0"], tab["w1"] = rec, win[:, 0], win[:, 1]
        with torch.cuda.device(dev):
            counts = torch.empty(N, 4, dtype=torch.int32, device=dev)
            stats = torch.empty(N, 10, dtype=torch.float32, device=dev)
            out = torch.empty(N, g["F"], dtype=torch.float32, device=dev) if psd else None
            if N:
                tab_dev = table_buffer(tab, dev)
                _lib.check(_lib.lib().ral_hrv_windows(_ptr(pos), None if label is None else _ptr(label), _ptr(count), pos.shape[0],
                                                      pos.shape[1], tab.ctypes.data, N, _ptr(tab_dev), 1, self.geom,
                                                      _ptr(self.band), _ptr(counts), _ptr(stats), None if out is None else _ptr(out),
                                                      _stream()))
        return HrvWindows(counts, stats, out, np.asarray(index, dtype=np.int64).reshape(N, 2), g)


def _labels(classes, pos, count, what="HrvAnalyzer.analyse"):
    """`BeatClasses`, per-record label lists or None -> (R, cap) int32 on the device of `pos`, or None; `what` is the caller's
    name in the messages"""
    if classes is None:
        return None
    if isinstance(classes, BeatClasses):
        lab = classes.label
        if lab.shape != pos.shape or lab.device != pos.device or lab.dtype != torch.int32:
            raise _lib.RalError(f"{what}: labels of shape {tuple(lab.shape)} on {lab.device} for beats of shape "
                                f"{tuple(pos.shape)} on {pos.device}")
        return lab.contiguous()
    rows = [np.asarray(r.cpu() if torch.is_tensor(r) else r, dtype=np.int64).reshape(-1) for r in classes]
    if len(rows) != pos.shape[0] or [len(r) for r in rows] != count.tolist():
        raise _lib.RalError(f"{what}: one label per beat of every record")
    return torch.from_numpy(pad_rows(rows, -1, shape=tuple(pos.shape))).to(pos.device)


class HrvAnalyzer:
    """HRV of whole records at rate `fs` (`ral_hrv_windows`).  `analyse(beats, T, classes=None, psd=False)` takes the beats of
    R records of T samples - a `Beats`, which is trusted, or per-record lists of strictly ascending positions in [0, T), which are
    checked on the host - and their labels - a `BeatClasses`, per-record lists, or None: every beat is N - and returns the
    `HrvWindows` of all records, record by record, window by window."""

    def __init__(self, fs=MODEL_RATE, win_s=300, hop_s=60, nn_range=(0.3, 2.0), fmax=Fraction(2, 5), min_nn=16, device="cuda"):
        self.fs, self.geometry = fs, hrv_check(hrv_geometry(fs, win_s, hop_s, nn_range, fmax, min_nn))
        self.engine = _Engine(self.geometry, device)
        self.device = self.engine.device

    @torch.no_grad()
    def analyse(self, beats, T, classes=None, psd=False):
        if isinstance(T, bool) or not isinstance(T, numbers.Integral) or not 1 <= T < 2 ** 31:
            raise _lib.RalError(f"HrvAnalyzer.analyse: T must be in [1, 2^31) (got {T!r})")
        pos, count = beat_lists(beats, self.device, "HrvAnalyzer.analyse", T=int(T))
        label = _labels(classes, pos, count)
        win = hrv_windows(T, self.geometry)
        R, nw = pos.shape[0], len(win)
        rec = np.repeat(np.arange(R, dtype=np.int64), nw)
        index = np.stack([rec, np.tile(np.arange(nw, dtype=np.int64), R)], axis=1)
        return self.engine.run(pos, label, count, rec, np.tile(win, (R, 1)), index, psd)


class HrvPoolState:
    """The host side of an `HrvPool`, without a device.  Per slot: the released beats, with labels, from the origin of the next
    unemitted window onwards (`pos`, `lab`), and the number of windows emitted so far (`emitted`).  `feed(beats, close)` takes
    {sid: (positions, labels)}, the beats a call has released in ascending order, and {sid: T}, the streams that end with it at
    length T, and returns per sid named (first window number, (n, 2) int64 windows [w0, w1) that became final, the positions and
    labels those windows are read from).  An open stream's window w is final once a released beat lies at or beyond w H + W; a
    closing stream's remaining windows w < max(1, (T - W) // H + 1) are all final, w1 clipped to T.  A call that raises has
    changed nothing."""

    def __init__(self, capacity, geometry, name="HrvPool"):
        self.geometry, self.capacity, self.name = hrv_check(geometry), int(capacity), name
        self.pos = [np.zeros(0, dtype=np.int64) for _ in range(self.capacity)]
        self.lab = [np.zeros(0, dtype=np.int32) for _ in range(self.capacity)]
        self.emitted = np.zeros(self.capacity, dtype=np.int64)
        self.last = np.full(self.capacity, -1, dtype=np.int64)         # the last released beat
        self.is_open = np.zeros(self.capacity, dtype=bool)

    def open(self, sid):
        if not (isinstance(sid, (int, np.integer)) and not isinstance(sid, bool) and 0 <= sid < self.capacity) or self.is_open[sid]:
            raise _lib.RalError(f"{self.name}.open: {sid!r} is not a free slot")
        self.pos[sid], self.lab[sid] = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32)
        self.emitted[sid], self.last[sid], self.is_open[sid] = 0, -1, True

    def feed(self, beats, close=None):
        close = dict(close or {})
        W, H = self.geometry["W"], self.geometry["H"]
        new = {}
        for sid in list(beats) + [s for s in close if s not in beats]:
            if not (isinstance(sid, (int, np.integer)) and not isinstance(sid, bool) and 0 <= sid < self.capacity
                    and self.is_open[sid]):
                raise _lib.RalError(f"{self.name}: {sid!r} is not an open stream")
            p, l = beats.get(sid, ((), ()))
            p, l = np.asarray(p, dtype=np.int64).reshape(-1), np.asarray(l, dtype=np.int32).reshape(-1)
            if len(p) != len(l):
                raise _lib.RalError(f"{self.name}: stream {sid}: {len(p)} positions with {len(l)} labels")
            if len(p) and (p[0] <= self.last[sid] or np.any(np.diff(p) <= 0)):
                raise _lib.RalError(f"{self.name}: stream {sid}: beats are released in strictly ascending order")
            if sid in close:
                T = close[sid]
                if isinstance(T, bool) or not isinstance(T, (int, np.integer)) or T < 1 or T <= max(self.last[sid], p[-1] if len(p) else -1):
                    raise _lib.RalError(f"{self.name}: stream {sid} ends at T={T!r}: need T >= 1, beyond its last beat")
            new[sid] = (p, l)
        out = {}
        for sid, (p, l) in new.items():
            pos, lab = np.concatenate([self.pos[sid], p]), np.concatenate([self.lab[sid], l])
            w_first = int(self.emitted[sid])
            if sid in close:
                T = int(close[sid])
                w_end = max(1, (T - W) // H + 1)
            else:
                T = None
                w_end = (int(pos[-1]) - W) // H + 1 if len(pos) and pos[-1] >= W else 0       # windows w with w H + W <= the last beat
            w_end = max(w_end, w_first)
            w0 = np.arange(w_first, w_end, dtype=np.int64) * H
            w1 = w0 + W if T is None else np.minimum(w0 + W, T)
            out[sid] = (w_first, np.stack([w0, w1], axis=1), pos, lab)
            if sid in close:
                self.pos[sid], self.lab[sid] = pos[:0], lab[:0]
                self.is_open[sid] = False
            else:
                keep = pos >= w_end * H
                self.pos[sid], self.lab[sid], self.emitted[sid] = pos[keep], lab[keep], w_end
                if len(p):
                    self.last[sid] = p[-1]
        return out


class HrvPool(StreamSurface):
    """HRV of up to `capacity` independent live streams of `leads` leads at rate `fs`, chunk by chunk: it owns a `BeatClassPool`
    (`classes`) and analyses the windows that its beats complete (`ral_hrv_windows`).  `open()` returns a stream id;
    `push(chunks, close=())` takes {sid: (leads, c)} (c >= 0, host or device) for any subset of the open streams, ends the streams
    listed in `close`, and returns {sid: HrvWindows} for every sid named: the windows that became final with this call, possibly
    none (`index` holds the sid and the window's number).  A window is final once a beat at or beyond its end has been released
    (the classifier holds the first eight beats of a stream until the ninth), or when the stream closes.  A push plans once, runs
    the `BeatClassPool` (its `run`, which synchronises), copies the new (position, label) pairs to the host, plans the final windows
    (`HrvPoolState`), uploads each affected stream's kept beats as one row - int32 positions relative to the origin of the first
    window the call emits for it - and calls `ral_hrv_windows` once.  Concatenated per stream from `open` to `close`, the windows
    equal those of `HrvAnalyzer.analyse(BeatDetector.detect(record), T, BeatClassifier.classify(record, beats))` bit for bit,
    whatever the chunking and the other streams.  Every argument is checked on the host before any device work; a call that
    raises has changed nothing.  (One limit: the windows a call emits for one stream, and the beats they read, must lie within
    2^31 samples of each other.)"""

    def __init__(self, leads, capacity, fs=MODEL_RATE, win_s=300, hop_s=60, nn_range=(0.3, 2.0), fmax=Fraction(2, 5), min_nn=16,
                 c0=0.7, r0=0.8, alpha=0.35, floor=0.0, band=(8, 24), device="cuda"):
        name = type(self).__name__
        self.geometry = hrv_check(hrv_geometry(fs, win_s, hop_s, nn_range, fmax, min_nn))
        self.classes = BeatClassPool(leads, capacity, fs, c0, r0, alpha, floor, band, device)
        self.state = self.classes.beats.state                       # the slots (`StreamSurface`)
        self.hrv = HrvPoolState(self.classes.capacity, self.geometry, name)
        self.engine = _Engine(self.geometry, self.classes.device)
        self.fs, self.leads, self.capacity, self.device = fs, self.classes.leads, self.classes.capacity, self.classes.device

    def open(self):
        sid = self.classes.open()
        self.hrv.open(sid)
        return sid

    @torch.no_grad()
    def push(self, chunks, close=()):
        close = tuple(close)
        xs = as_chunks(chunks)
        sids, btab = self.classes.state.plan({sid: tuple(x.shape) for sid, x in xs.items()}, close)      # (raises before anything changes)
        ends = {sid: int(n0 + c) for sid, n0, c, T in zip(sids, btab["n0"], btab["c"], btab["T"]) if T >= 0}
        xp, x_total, _ = pack_chunks(xs, self.leads, self.device)
        res = self.classes.run(xp, x_total, sids, btab)                # (its `run`, never its `push`: the call is planned once)
        n = [res[sid][0].numel() for sid in sids]
        if sum(n):
            p = torch.cat([res[sid][0] for sid in sids]).cpu().numpy()
            l = torch.cat([res[sid][1] for sid in sids]).cpu().numpy()
        else:
            p, l = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32)
        o = np.cumsum([0] + n)
        plan = self.hrv.feed({sid: (p[o[i]:o[i + 1]], l[o[i]:o[i + 1]]) for i, sid in enumerate(sids)}, ends)
        g, rows, labs, rec, win, index, nrow = self.geometry, [], [], [], [], [], []
        for sid in sids:
            w_first, w, pos, lab = plan[sid]
            nrow.append(len(w))
            if not len(w):
                continue
            origin = w_first * g["H"]
            use = pos < w[-1, 1]
            if w[-1, 1] - origin >= 2 ** 31:
                raise _lib.RalError(f"{type(self).__name__}.push: the windows this call completes for stream {sid} span 2^31 samples")
            rec += [len(rows)] * len(w)
            rows.append(pos[use] - origin)
            labs.append(lab[use])
            win.append(w - origin)
            index += [(sid, w_first + i) for i in range(len(w))]
        if rows:
            dev = self.device
            pos_d = torch.from_numpy(pad_rows(rows, -1)).to(dev)
            lab_d = torch.from_numpy(pad_rows(labs, -1)).to(dev)
            cnt_d = torch.tensor([len(r) for r in rows], dtype=torch.int32, device=dev)
            allw = self.engine.run(pos_d, lab_d, cnt_d, np.asarray(rec, dtype=np.int64), np.concatenate(win), index, False)
        else:
            allw = self.engine.run(torch.zeros(1, 1, dtype=torch.int32, device=self.device), None, None, np.zeros(0, dtype=np.int64),
                                   np.zeros((0, 2), dtype=np.int64), np.zeros((0, 2), dtype=np.int64), False)
        out, at = {}, 0
        for sid, k in zip(sids, nrow):
            out[sid] = HrvWindows(allw.counts[at:at + k], allw.stats[at:at + k], None, allw.index[at:at + k], g)
            at += k
        return out


METRICS = ("hr", "sdnn", "rmssd", "log_lf_hf")


class HrvEvaluation:
    """What `evaluate_hrv` returns: `clean`, `noisy`, `denoised`, the `HrvWindows` of the three records (the same windows in the
    same order); `errors` = {"noisy": {metric: mean absolute error against the clean windows}, "denoised": {...}} for the
    metrics hr, sdnn, rmssd and log_lf_hf = log(lf_hf), each over the windows where the clean, the noisy and the denoised value
    are all finite (NaN if there is none), and `windows` = {metric: how many those are}."""

    def __init__(self, clean, noisy, denoised, errors, windows):
        self.clean, self.noisy, self.denoised, self.errors, self.windows = clean, noisy, denoised, errors, windows


def _metric(h, name):
    return torch.log(h.lf_hf.double()) if name == "log_lf_hf" else getattr(h, name).double()


def evaluate_hrv(denoiser, records, noise, snr_db, offsets=None, rng=None, detector=None, classifier=None, analyzer=None):
    """The noise-stress protocol scored in rhythm statistics: `mix_records(records, noise, snr_db, offsets, rng)`,
    `denoiser.denoise(noisy)`, then the clean, the noisy and the denoised records are each detected, classified and analysed ON
    THEIR OWN - unlike `evaluate_rhythm`, the beat positions are part of what the noise damages - and per metric (hr, sdnn, rmssd,
    log(lf_hf)) the mean absolute error of the noisy and of the denoised windows against the clean record's is taken over the
    windows where all three values are finite -> `HrvEvaluation`.  `denoiser` is a `StreamingDenoiser` or a
    `RateStreamingDenoiser`; detector, classifier and analyzer (defaults `BeatDetector(fs)`, `BeatClassifier(fs)`,
    `HrvAnalyzer(fs)`) run at that object's outer rate `fs`."""
    fs, dev, clean, noisy, out = stress_front(denoiser, records, noise, snr_db, offsets, rng)
    det, cls = detector or BeatDetector(fs, device=dev), classifier or BeatClassifier(fs, device=dev)
    ana = analyzer or HrvAnalyzer(fs, device=dev)
    hs = []
    for x in (clean, noisy, out):
        beats = det.detect(x)
        hs.append(ana.analyse(beats, x.shape[-1], cls.classify(x, beats)))
    errors, windows = {"noisy": {}, "denoised": {}}, {}
    for name in METRICS:
        c, a, b = (_metric(h, name) for h in hs)
        ok = torch.isfinite(c) & torch.isfinite(a) & torch.isfinite(b)
        windows[name] = int(ok.sum())
        for key, v in (("noisy", a), ("denoised", b)):
            errors[key][name] = float((v[ok] - c[ok]).abs().mean()) if windows[name] else float("nan")
    return HrvEvaluation(hs[0], hs[1], hs[2], errors, windows)
