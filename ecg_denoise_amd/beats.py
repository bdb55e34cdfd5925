"""R-peak detection on the device: the step every consumer of a denoised ECG takes next.

    beats = BeatDetector(fs=360).detect(records)            # whole records, ral_beat_records -> Beats (peaks, count)
    pool = BeatPool(leads, capacity, fs=360)                # chunks of independent streams, ral_beat_pool
    scores = match_beats(ref, beats, tol_s=0.15, fs=360)    # ral_beat_match -> tp / fp / fn, Se, +P, F1
    ev = evaluate_beats(denoiser, records, noise, snr_db)   # the noise-stress protocol scored in beats, before / after

The detector (include/ralenet.h has the same definition).  Input (R, leads, T) fp32 at rate fs; one beat list per record, all
leads contribute.  Lengths in samples, derived here from seconds (`beat_geometry`; round = nearest, halves up, exact):

    half = round(0.25 fs) = 90 at 360 Hz;  Wi = round(0.075 fs) = 27;  Wt = round(1.5 fs) = 540;  Rf = round(0.2 fs) = 72;
    Rw = round(0.075 fs) = 27;  alpha = 0.35, floor = 0, band 8-24 Hz

    k = -half .. half
    h[k+half] = ((2 f_hi/fs) sinc(2 f_hi k/fs) - (2 f_lo/fs) sinc(2 f_lo k/fs)) * np.hamming(2 half + 1)[k+half]
    h -= mean(h)                                           # designed in fp64 with numpy (`beat_bank`), passed as fp32
    y_l[n] = sum over k ascending of h[k+half] * x_l[clamp(n - k, 0, T-1)]      # fp32, fmaf, edge-replicated
    f[n]   = sum over leads in lead order of y_l[n]^2
    m[n]   = (sum over j = -Wi .. Wi ascending of f[n+j], f = 0 outside [0,T)) / (2 Wi + 1)
    thr[n] = max(alpha * max over |j| <= Wt of m[n+j] (clipped to [0,T)), floor)
    n is a candidate iff m[n] > 0, m[n] >= thr[n], m[n] > m[n+j] for -Rf <= j < 0 and m[n] >= m[n+j] for 0 < j <= Rf (clipped)
    peak(n) = lowest index attaining max of f over [n-Rw, n+Rw] (clipped)

Per record the peaks ascend; int32, padded with -1 to cap = T // (Rf + 1) + 1, plus a count.  Every value is computed
independently of its neighbours in a fixed order - no running sums, no adaptive state carried along the record - so the work is
parallel over time and a stream processed in chunks gives exactly the integers of the complete record.  A decision at n is
final once sample n + Wt + Wi + half has been received or the stream has closed: `beat_frontier(n_in)` decisions after n_in
samples, `beat_latency(fs)` seconds (657 samples, 1.83 s, at 360 Hz).

Non-finite samples are out of scope: the peaks of a record that holds a NaN or an infinity are undefined.  With floor = 0 the
threshold is relative only: every record that is not exactly silent yields detections, a constant one among them (its fp32
rounding residue is its "signal"); a floor, in units of m (squared filtered amplitude), removes them.  The defaults were chosen
on synthetic data (`synth`) only; none has been tuned on MIT-BIH.

Device tensors only: there is no CPU fallback."""
from fractions import Fraction

import numpy as np
import torch

from . import _lib
from .evaluate import stress_front
from .intake import Beats, beat_lists, check_leads, device_records, record_shape
from .model import _ptr, _stream
from .pools import SlotState, StreamSurface, as_chunks, pack_chunks, scratch_bytes, table_buffer
from .rate import _rate

MODEL_RATE = 360
AAMI_TOL_S = 0.15        # ANSI/AAMI EC57: a detection within 150 ms of a reference beat matches it

# the LDS budget of ral_beats.hip (beat_geom there): a feature workgroup forms _FN_MAX values of f, halved down to _FN_MIN while
# the bank, the spans of all leads and those values exceed _LDS_FLOATS floats; a pick workgroup holds three arrays of
# _PICK + 2 Wt floats
_FN_MAX, _FN_MIN, _PICK, _LDS_FLOATS, _THREADS = 1024, 128, 1024, 16384, 256


def _round(v):
    return int((v + Fraction(1, 2)).__floor__())


def beat_geometry(fs=MODEL_RATE):
    """-> {half, Wi, Wt, Rf, Rw} in samples at rate `fs` (a positive int or Fraction)"""
    fs = _rate(fs, "fs")
    return {"half": _round(fs / 4), "Wi": _round(fs * 3 / 40), "Wt": _round(fs * 3 / 2), "Rf": _round(fs / 5),
            "Rw": _round(fs * 3 / 40)}


def beat_bank(fs=MODEL_RATE, f_lo=8, f_hi=24):
    """the 2 half + 1 taps of the band-pass f_lo .. f_hi Hz at rate `fs`, fp64: a Hamming-windowed difference of two sincs with
    its mean removed (symmetric, zero DC gain)"""
    half = beat_geometry(fs)["half"]
    fs = float(_rate(fs, "fs"))
    if not (0 < f_lo < f_hi < fs / 2):
        raise _lib.RalError(f"beat_bank: need 0 < f_lo < f_hi < fs / 2 (got {f_lo}, {f_hi} at {fs} Hz)")
    k = np.arange(-half, half + 1, dtype=np.float64)
    h = ((2 * f_hi / fs) * np.sinc(2 * f_hi * k / fs) - (2 * f_lo / fs) * np.sinc(2 * f_lo * k / fs)) * np.hamming(2 * half + 1)
    return h - h.mean()


def _lag(g):
    return g["Wt"] + g["Wi"] + g["half"]


def beat_frontier(n_in, fs=MODEL_RATE):
    """decisions that are final once a stream has received n_in samples, whatever follows: decision n is final iff
    n + Wt + Wi + half < n_in, so max(0, n_in - (Wt + Wi + half))"""
    return max(0, int(n_in) - _lag(beat_geometry(fs)))


def beat_latency(fs=MODEL_RATE):
    """seconds a decision waits after its own instant: (Wt + Wi + half) / fs"""
    return float(_lag(beat_geometry(fs)) / _rate(fs, "fs"))


def beat_check(fs, leads):
    """raise RalError unless the detector's spans for `leads` leads at rate `fs` fit the kernels' LDS budget -> the geometry"""
    g = beat_geometry(fs)
    check_leads(leads, "beat detection")
    nt4 = (2 * g["half"] + 1 + 3) // 4 * 4
    ok = 1 <= g["half"] <= 8192 and 1 <= g["Rf"] <= g["Wt"] and 2 * g["Rw"] <= g["Rf"] and g["Rw"] <= g["Wt"] + g["Wi"]
    ok = ok and 3 * (_PICK + 2 * g["Wt"]) + _THREADS <= _LDS_FLOATS
    fn = _FN_MAX
    while ok and fn >= _FN_MIN and not (leads * (fn + nt4) + nt4 + fn <= _LDS_FLOATS and 2 * (fn - 2 * g["Wi"]) >= fn):
        fn //= 2
    if not ok or fn < _FN_MIN:
        raise _lib.RalError(f"beat detection at fs={fs} with {leads} leads is not supported: the filter bank ({nt4} taps), the input "
                            f"span of all leads of one tile and the threshold window ({2 * g['Wt'] + 1} samples) do not fit the "
                            f"kernels' {_LDS_FLOATS * 4 // 1024} KB of LDS")
    return g


class _Detector:
    """the geometry, the thresholds and the bank of one detector on one device"""

    def __init__(self, fs, alpha, floor, band, leads, device, what):
        self.fs, self.alpha, self.floor, self.band = fs, float(alpha), float(floor), tuple(band)
        if not (np.isfinite(self.alpha) and self.alpha > 0 and np.isfinite(self.floor) and self.floor >= 0):
            raise _lib.RalError(f"{what}: need a finite alpha > 0 and floor >= 0 (got alpha={alpha!r} floor={floor!r})")
        self.geometry = beat_geometry(fs) if leads is None else beat_check(fs, leads)
        g = self.geometry
        self.geom = _lib.BeatGeom(g["half"], g["Wi"], g["Wt"], g["Rf"], g["Rw"], self.alpha, self.floor, 0)
        self.lag = _lag(g)
        self.bank_host = beat_bank(fs, *self.band).astype(np.float32)
        self.device = torch.device(device)
        self.bank = None

    def on_device(self):
        if self.bank is None:
            self.bank = torch.from_numpy(self.bank_host).to(self.device)
        return self.bank


class BeatDetector:
    """R peaks of whole records at rate `fs` (`ral_beat_records`).  `detect(records)` takes a device tensor (leads, T) or
    (R, leads, T) and returns `Beats`; the filter bank is designed and uploaded once per instance."""

    def __init__(self, fs=MODEL_RATE, alpha=0.35, floor=0.0, band=(8, 24), device="cuda"):
        self.det = _Detector(fs, alpha, floor, band, None, device, "BeatDetector")
        self.fs, self.geometry = fs, self.det.geometry

    def cap(self, T):
        """columns of `Beats.peaks` for records of T samples"""
        return int(T) // (self.geometry["Rf"] + 1) + 1

    @torch.no_grad()
    def detect(self, records):
        R, leads, T = record_shape(records, "BeatDetector.detect")
        beat_check(self.fs, leads)
        x = device_records(records, "BeatDetector.detect")
        d, lib, cap = self.det, _lib.lib(), self.cap(T)
        d.device = x.device if d.bank is None else d.device
        if x.device != d.device:
            raise _lib.RalError(f"BeatDetector.detect: the records are on {x.device}, the detector's bank on {d.device}")
        nbytes = scratch_bytes(lib.ral_beat_records_scratch_bytes(R, leads, T, d.geom))
        with torch.cuda.device(x.device):
            scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=x.device)
            peaks = torch.empty(R, cap, dtype=torch.int32, device=x.device)
            count = torch.empty(R, dtype=torch.int32, device=x.device)
            _lib.check(lib.ral_beat_records(_ptr(x), R, leads, T, d.geom, _ptr(d.on_device()), d.bank_host.size, _ptr(scratch),
                                            scratch.numel() * 8, _ptr(peaks), cap, _ptr(count), _stream()))
        return Beats(peaks, count, self.fs)


class BeatPoolState(SlotState):
    """The host side of a `BeatPool`, without a device: the slots (`SlotState`) and the detector's geometry.  `plan` checks the
    arguments of a call and builds its table (`_lib.BEAT_ROW`) without changing anything; `commit` applies a planned call.
    After n samples the decisions [0, frontier(n)) of a stream have been made; closing it at T makes the rest, up to T."""

    def __init__(self, leads, capacity, fs=MODEL_RATE, name="BeatPool"):
        self.geometry = beat_check(fs, leads)
        super().__init__(capacity, leads, name)
        self.fs, self.lag = fs, _lag(self.geometry)
        self.hist_len = 2 * self.lag

    def frontier(self, n):
        return max(0, int(n) - self.lag)

    def plan(self, shapes, close=()):
        """shapes {sid: shape of its chunk, (leads, c) with c >= 0}, close: the sids that end with this call -> (sids in row
        order, table); raises RalError for a bad argument"""
        named = self.named(shapes, close, 65535, "65535 streams")
        sids, _, lens, ends, n0 = named
        tab = self.rows(_lib.BEAT_ROW, named, need_sample=True)
        n1 = n0 + lens
        d0 = np.maximum(0, n0 - self.lag)
        d = np.where(ends, n1, np.maximum(0, n1 - self.lag)) - d0
        cap = np.where(d > 0, d // (self.geometry["Rf"] + 1) + 1, 0)
        tab["d0"], tab["d"], tab["cap"], tab["out_off"] = d0, d, cap, np.cumsum(cap) - cap
        return sids, tab

    def span(self, tab):
        """the longest span of f that a row of the table reads (what the call's scratch is sized by), at least 1"""
        w = self.geometry["Wt"] + self.geometry["Wi"]
        d0, d1 = tab["d0"], tab["d0"] + tab["d"]
        s = np.where(tab["d"] > 0, np.minimum(tab["n0"] + tab["c"], d1 + w) - np.maximum(0, d0 - w), 0)
        return max(1, int(s.max()))

    commit = SlotState.commit_rows


class BeatPool(StreamSurface):
    """R peaks of up to `capacity` independent live streams of `leads` leads at rate `fs`, chunk by chunk (`ral_beat_pool`).
    `open()` returns a stream id; `push(chunks, close=())` takes {sid: (leads, c)} (c >= 0, host or device) for any subset of the
    open streams, ends the streams listed in `close`, and returns {sid: int64 device tensor} for every sid named: the peaks of
    the decisions that became final with this call, as absolute sample indices of the stream, ascending.  After n samples the
    decisions [0, beat_frontier(n, fs)) have been made; closing a stream makes the rest with the record's end rules.
    Concatenated per stream from `open` to `close`, the results equal `BeatDetector.detect(record)` integer for integer,
    whatever the chunking and the other streams.  (A peak lies within Rw of its decision, so it may precede the frontier of the
    call before - never a peak already given.)  `close(sid, x=None)` ends one stream.  Every argument is checked on the host
    before any device work (`plan`); a call that raises has changed nothing.  A slot keeps its last 2 (Wt + Wi + half) raw
    samples on the device, in two planes used in turn; f and m are formed again for the span each call's decisions read.
    `push` synchronises (the number of peaks sizes its results)."""

    def __init__(self, leads, capacity, fs=MODEL_RATE, alpha=0.35, floor=0.0, band=(8, 24), device="cuda"):
        self.state = BeatPoolState(leads, capacity, fs, type(self).__name__)
        self.det = _Detector(fs, alpha, floor, band, leads, device, type(self).__name__)
        self.fs, self.leads, self.capacity, self.hist_len = fs, self.state.leads, self.state.capacity, self.state.hist_len
        self.geometry, self.device = self.state.geometry, self.det.device
        self.det.on_device()
        self.hist = torch.zeros(2, self.capacity, self.leads, self.hist_len, dtype=torch.float32, device=self.device)

    def plan(self, shapes, close=()):
        return self.state.plan(shapes, close)

    @torch.no_grad()
    def push(self, chunks, close=()):
        xs = as_chunks(chunks)
        sids, tab = self.state.plan({sid: tuple(x.shape) for sid, x in xs.items()}, tuple(close))
        xp, x_total, _ = pack_chunks(xs, self.leads, self.device)
        return self.run(xp, x_total, sids, tab)

    def run(self, xp, x_total, sids, tab):
        """carry out a planned call: xp, x_total the chunks as `pack_chunks` packs them, sids and tab as planned ->
        {sid: peaks}; commits the plan"""
        dev, leads, d, lib = self.device, self.leads, self.det, _lib.lib()
        peaks_total = int(tab["cap"].sum())
        nbytes = scratch_bytes(lib.ral_beat_records_scratch_bytes(len(tab), leads, self.state.span(tab), d.geom))
        with torch.cuda.device(dev):
            scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=dev)
            peaks = torch.empty(max(peaks_total, 1), dtype=torch.int64, device=dev)
            count = torch.empty(len(tab), dtype=torch.int32, device=dev)
            tab_dev = table_buffer(tab, dev)
            _lib.check(lib.ral_beat_pool(_ptr(self.hist), _ptr(xp), x_total, tab.ctypes.data, len(tab), _ptr(tab_dev), 1,
                                         self.capacity, leads, d.geom, _ptr(d.bank), d.bank_host.size, self.hist_len,
                                         _ptr(scratch), scratch.numel() * 8, _ptr(peaks), peaks_total, _ptr(count), _stream()))
        self.state.commit(tab)
        return {sid: peaks[o:o + n] for sid, o, n in zip(sids, tab["out_off"].tolist(), count.tolist())}


class BeatScores:
    """What `match_beats` returns: `tp`, `fp`, `fn` (R,) int64 device tensors, and from them per record `sensitivity`
    tp / (tp + fn), `ppv` tp / (tp + fp) and `f1` 2 tp / (2 tp + fp + fn) as float64 device tensors (NaN where the denominator
    is 0); `pooled` gives the same six over the sums of all records, as plain numbers (synchronises)."""

    def __init__(self, counts, tol):
        self.counts, self.tol = counts, int(tol)            # (R, 3) int64: tp, fp, fn
        self.tp, self.fp, self.fn = counts[:, 0], counts[:, 1], counts[:, 2]

    @staticmethod
    def _ratios(tp, fp, fn):
        return tp / (tp + fn), tp / (tp + fp), 2 * tp / (2 * tp + fp + fn)

    sensitivity = property(lambda self: self._ratios(*self.counts.double().unbind(1))[0])
    ppv = property(lambda self: self._ratios(*self.counts.double().unbind(1))[1])
    f1 = property(lambda self: self._ratios(*self.counts.double().unbind(1))[2])

    @property
    def pooled(self):
        tp, fp, fn = self.counts.sum(0).tolist()
        with np.errstate(invalid="ignore", divide="ignore"):
            se, pp, f1 = (float(v) for v in self._ratios(np.float64(tp), np.float64(fp), np.float64(fn)))
        return {"tp": tp, "fp": fp, "fn": fn, "sensitivity": se, "ppv": pp, "f1": f1}


def match_beats(ref, det, tol_s=AAMI_TOL_S, fs=MODEL_RATE, device=None):
    """`ref` and `det`: `Beats`, or per record one ascending list (or tensor) of sample indices -> `BeatScores` (`ral_beat_match`).
    Per record the two lists are walked together: ref[i] and det[j] match iff |det - ref| <= tol = floor(tol_s fs) samples,
    otherwise the smaller index advances.  150 ms is the AAMI EC57 convention.  Runs on the device of the `Beats` given, else on
    `device` (default "cuda")."""
    dev = next((b.peaks.device for b in (ref, det) if isinstance(b, Beats)), torch.device(device or "cuda"))
    if dev.type != "cuda":
        raise _lib.RalError("match_beats runs on the GPU (there is no CPU fallback)")
    tol = int((Fraction(str(tol_s)) * _rate(fs, "fs")).__floor__())
    if tol < 0:
        raise _lib.RalError(f"match_beats: tol_s must be >= 0 (got {tol_s!r})")
    (rp, rc), (dp, dc) = (beat_lists(b, dev, "match_beats", strict=False, name=n) for b, n in ((ref, "ref"), (det, "det")))
    if rp.shape[0] != dp.shape[0] or rp.device != dp.device:
        raise _lib.RalError(f"match_beats: ref has {rp.shape[0]} records on {rp.device}, det {dp.shape[0]} on {dp.device}")
    with torch.cuda.device(dev):
        out = torch.empty(rp.shape[0], 3, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().ral_beat_match(_ptr(rp), _ptr(rc), rp.shape[1], _ptr(dp), _ptr(dc), dp.shape[1], rp.shape[0], tol,
                                             _ptr(out), _stream()))
    return BeatScores(out, tol)


class BeatEvaluation:
    """What `evaluate_beats` returns: `noisy` and `denoised`, the `BeatScores` of the detections on the noisy and on the
    denoised records against `ref`; `ref`, `det_noisy`, `det_denoised` are the lists themselves."""

    def __init__(self, noisy, denoised, ref, det_noisy, det_denoised):
        self.noisy, self.denoised, self.ref, self.det_noisy, self.det_denoised = noisy, denoised, ref, det_noisy, det_denoised


def evaluate_beats(denoiser, records, noise, snr_db, ref=None, offsets=None, rng=None, tol_s=AAMI_TOL_S, detector=None):
    """The noise-stress protocol scored in beats: `mix_records(records, noise, snr_db, offsets, rng)`, `denoiser.denoise(noisy)`,
    detection on the clean, the noisy and the denoised records, `match_beats` of the last two against `ref` (`Beats` or per-record
    lists; default: the detections on the clean records) -> `BeatEvaluation`.  `denoiser` is a `StreamingDenoiser` or a
    `RateStreamingDenoiser`; the detector (default `BeatDetector(fs)`) runs at that object's outer rate `fs`, 360 Hz for a
    `StreamingDenoiser`."""
    fs, dev, clean, noisy, out = stress_front(denoiser, records, noise, snr_db, offsets, rng)
    det = detector or BeatDetector(fs, device=dev)
    ref = det.detect(clean) if ref is None else ref
    b_noisy, b_out = det.detect(noisy), det.detect(out)
    return BeatEvaluation(match_beats(ref, b_noisy, tol_s, fs), match_beats(ref, b_out, tol_s, fs), ref, b_noisy, b_out)
