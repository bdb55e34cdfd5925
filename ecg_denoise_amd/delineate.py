"""Beat delineation on the device: where do the QRS complex and the T wave of a detected beat begin and end?

    fid = BeatDelineator(fs=360).delineate(records, beats)         # whole records, ral_delineate_records -> Fiducials
    fid.qrs_ms(), fid.qt_ms(), fid.qtc_ms()                        # the intervals a clinical reader takes from them
    ev = evaluate_intervals(denoiser, records, noise, snr_db)      # the noise-stress protocol scored in intervals

The delineator (include/ralenet.h has the same definition).  Input (R, leads, T) fp32 at rate fs and, per record, strictly
ascending beat positions p_0 < ... < p_{n-1} in [0, T): a `Beats` from `BeatDetector`, or per-record lists such as annotations.
c(t) = clamp(t, 0, T - 1).  Lengths in samples (`delineate_geometry`; the rounding of `beat_geometry`: nearest, halves up, exact):

    h = max(1, round(fs / 180)) = 2 at 360 Hz;  m = round(fs / 120) = 3;  Wq = round(0.12 fs) = 43;  g = round(fs / 50) = 7;
    m2 = round(fs / 60) = 6;  gt = round(0.06 fs) = 22;  Wt = round(0.55 fs) = 198

All floating arithmetic is fp32, every sum is taken one term at a time in the order written, and no product is ever followed by
an addition, so nothing can contract into an FMA: the four integers of a beat are reproducible bit for bit.

    slope activity   d[t] = sum_l |x_l[c(t + h)] - x_l[c(t - h)]|, in lead order
    smoothed slope   a[t] = sum_{k = -m .. m} d[c(t + k)], k ascending

QRS bounds of beat i at p = p_i: lo = max(p - Wq, 0), hi = min(p + Wq, T - 1); A = max a[t] over [lo, hi]; theta = q0 A, one fp32
product (default q0 = 0.15).  A == 0: all four points are -1.

    on       the largest t in [lo, p] with t - g >= 0 and a[t - j] <= theta for every j = 1 .. g; none: -1
    off      the smallest t in [p, hi] with t + g <= T - 1 and a[t + j] <= theta for every j = 1 .. g; none: -1

The T wave is measured only if on >= 0 and off >= 0: lim = min(p + Wt, T - 1), and when beat i + 1 exists lim is also capped at
p + (2 (p_{i+1} - p)) // 3; t0 = off + gt; t0 > lim: tpeak = tend = -1.

    smoothed leads   z_l[t] = sum_{k = -m2 .. m2} x_l[c(t + k)]; the isoelectric level of a lead is b_l = z_l[on]
    deviation        s[t] = sum_l |z_l[t] - b_l|, in lead order
    tpeak            the first argmax of s over [t0, lim]; that maximum 0, or tpeak == lim: tpeak = tend = -1
    tend             (the trapezium-area rule) the first argmax over t in [tpeak, lim] of
                     (s[tpeak] - s[t]) * float(2 lim - tpeak - t)

Every beat is measured on its own, by one wave: its result depends only on the record, its own position and the next beat's
position.

Non-finite samples are out of scope, as for the detector.  The defaults were chosen on synthetic data (`synth`) only; none has
been tuned on a database.

Device tensors only: there is no CPU fallback."""
import numpy as np
import torch

from . import _lib
from .beats import MODEL_RATE, BeatDetector, Beats, _round
from .evaluate import stress_front
from .intake import beat_lists, check_leads, device_records, record_shape
from .model import _ptr, _stream
from .rate import _rate

# the LDS budget of ral_delineate.hip (delin_geom there): a wave keeps d over [lo - g - m, hi + g + m], a over [lo - g, hi + g]
# and s over [t0, lim]
_LDS_BYTES = 65536


def delineate_geometry(fs=MODEL_RATE):
    """-> {h, m, Wq, g, m2, gt, Wt} in samples at rate `fs` (a positive int or Fraction)"""
    fs = _rate(fs, "fs")
    return {"h": max(1, _round(fs / 180)), "m": _round(fs / 120), "Wq": _round(fs * 3 / 25), "g": _round(fs / 50),
            "m2": _round(fs / 60), "gt": _round(fs * 3 / 50), "Wt": _round(fs * 11 / 20)}


def _lds_bytes(g):
    return 4 * (2 * (g["Wq"] + g["g"] + g["m"]) + 1 + 2 * (g["Wq"] + g["g"]) + 1 + g["Wt"] + 1)


def delineate_check(fs, leads):
    """raise RalError unless the delineator's windows at rate `fs` fit the kernel's LDS budget -> the geometry"""
    g = delineate_geometry(fs)
    check_leads(leads, "beat delineation", 65535)
    if g["Wq"] < 1 or g["g"] < 1 or g["Wt"] < 1 or _lds_bytes(g) > _LDS_BYTES:
        raise _lib.RalError(f"beat delineation at fs={fs} is not supported: the windows of one beat "
                            f"({2 * (g['Wq'] + g['g'] + g['m']) + 1}, {2 * (g['Wq'] + g['g']) + 1} and {g['Wt'] + 1} samples) "
                            f"do not fit the kernel's {_LDS_BYTES // 1024} KB of LDS")
    return g


class Fiducials:
    """What `BeatDelineator.delineate` returns: `on`, `off`, `tpeak`, `tend` (R, cap) int32 on the device, the QRS onset and
    offset, the T peak and the T end of every beat as sample indices, -1 where a point is undetermined or padding; `peaks`
    (R, cap) int32 are the positions that were measured, `count` (R,) int32 how many each record has, `fs` the rate the indices
    refer to.  The intervals are torch operations on these tensors: (R, cap) fp32, NaN where a point is missing."""

    def __init__(self, on, off, tpeak, tend, peaks, count, fs=MODEL_RATE):
        self.on, self.off, self.tpeak, self.tend, self.peaks, self.count, self.fs = on, off, tpeak, tend, peaks, count, fs

    def __len__(self):
        return self.on.shape[0]

    def tolist(self):
        """-> [(on, off, tpeak, tend) of record r, four plain lists of count[r] values] (synchronises)"""
        n = self.count.tolist()
        cols = [t.tolist() for t in (self.on, self.off, self.tpeak, self.tend)]
        return [tuple(c[r][:k] for c in cols) for r, k in enumerate(n)]

    def _ms64(self, a, b):
        """(b - a) 1000 / fs in fp64, NaN where either point is missing"""
        nan = torch.full(a.shape, float("nan"), dtype=torch.float64, device=a.device)
        return torch.where((a >= 0) & (b >= 0), (b - a).double() * 1000.0 / float(self.fs), nan)

    def _rr64(self):
        rr = torch.full(self.peaks.shape, float("nan"), dtype=torch.float64, device=self.peaks.device)
        i = torch.arange(1, self.peaks.shape[1], device=self.peaks.device)
        d = (self.peaks[:, 1:] - self.peaks[:, :-1]).double() / float(self.fs)
        rr[:, 1:] = torch.where(i[None, :] < self.count[:, None], d, rr[:, 1:])
        return rr

    def qrs_ms(self):
        """QRS duration (off - on) 1000 / fs in ms (formed in fp64, rounded once)"""
        return self._ms64(self.on, self.off).float()

    def qt_ms(self):
        """QT interval (tend - on) 1000 / fs in ms (formed in fp64, rounded once)"""
        return self._ms64(self.on, self.tend).float()

    def rr_s(self):
        """the RR interval to the previous beat in seconds; NaN for the first beat of a record and for padding"""
        return self._rr64().float()

    def qtc_ms(self):
        """Bazett's corrected QT in ms: QT in seconds over the square root of the RR to the previous beat in seconds (formed
        in fp64, rounded once); NaN for the first beat of a record"""
        return (self._ms64(self.on, self.tend) / torch.sqrt(self._rr64())).float()

    def measurable(self):
        """-> {"qrs": (R, cap) bool, on and off found; "qt": (R, cap) bool, on and tend found}"""
        return {"qrs": (self.on >= 0) & (self.off >= 0), "qt": (self.on >= 0) & (self.tend >= 0)}


class BeatDelineator:
    """QRS onset and offset, T peak and T end of the beats of whole records at rate `fs` (`ral_delineate_records`).
    `delineate(records, beats)` takes a device tensor (leads, T) or (R, leads, T) and the beats of every record - a `Beats`, or
    per-record lists of strictly ascending positions in [0, T), which are checked on the host - and returns `Fiducials`."""

    def __init__(self, fs=MODEL_RATE, q0=0.15, device="cuda"):
        self.fs, self.q0, self.geometry = fs, float(q0), delineate_geometry(fs)
        if not (np.isfinite(self.q0) and self.q0 >= 0):
            raise _lib.RalError(f"BeatDelineator: need a finite q0 >= 0 (got q0={q0!r})")
        g = self.geometry
        self.geom = _lib.DelinGeom(g["h"], g["m"], g["Wq"], g["g"], g["m2"], g["gt"], g["Wt"], self.q0)
        self.device = torch.device(device)

    @torch.no_grad()
    def delineate(self, records, beats):
        what = "BeatDelineator.delineate"
        R, leads, T = record_shape(records, what)
        delineate_check(self.fs, leads)
        peaks, count = beat_lists(beats, records.device, what, T=T, R=R)       # (the lists are checked on the host)
        x = device_records(records, what)
        cap = peaks.shape[1]
        with torch.cuda.device(x.device):
            on, off, tpeak, tend = (torch.empty(R, cap, dtype=torch.int32, device=x.device) for _ in range(4))
            _lib.check(_lib.lib().ral_delineate_records(_ptr(x), R, leads, T, self.geom, _ptr(peaks), _ptr(count), cap, _ptr(on),
                                                        _ptr(off), _ptr(tpeak), _ptr(tend), _stream()))
        return Fiducials(on, off, tpeak, tend, peaks, count, self.fs)


class IntervalEvaluation:
    """What `evaluate_intervals` returns: `clean`, `noisy`, `denoised`, the `Fiducials` of the three records at the same beats
    `ref`; `share` = {"noisy": {"qrs": (R,), "qt": (R,)}, "denoised": {...}}, per record the share of the beats measurable in the
    clean record that are measurable here too; `mae_ms` in the same layout, per record the mean absolute error of QRS duration
    and of QT in ms over the beats measurable in both (fp64 on the device, NaN where there is no such beat); `pooled` =
    {"noisy": {"qrs_share", "qt_share", "qrs_mae_ms", "qt_mae_ms", "qrs_beats", "qt_beats"}, "denoised": {...}}, the same over
    the beats of all records as plain numbers (`*_beats`: how many were measurable in both)."""

    def __init__(self, clean, noisy, denoised, ref, share, mae_ms, pooled):
        self.clean, self.noisy, self.denoised, self.ref = clean, noisy, denoised, ref
        self.share, self.mae_ms, self.pooled = share, mae_ms, pooled


def interval_scores(clean, other, rows=None):
    """the `Fiducials` of the clean records and of another condition at the same beats -> (share, mae_ms, pooled) as in
    `IntervalEvaluation`; `rows` (a bool or index tensor over the records) narrows the pooled values"""
    share, mae, pooled = {}, {}, {}
    mc, mo = clean.measurable(), other.measurable()
    keep = torch.ones(len(clean), dtype=torch.bool, device=clean.on.device)
    if rows is not None:
        keep = torch.zeros_like(keep)
        keep[rows] = True
    for key, fn in (("qrs", Fiducials.qrs_ms), ("qt", Fiducials.qt_ms)):
        both = mc[key] & mo[key]
        err = torch.where(both, (fn(other).double() - fn(clean).double()).abs(), torch.zeros((), dtype=torch.float64, device=both.device))
        nc, nb = mc[key].sum(1).double(), both.sum(1).double()
        share[key], mae[key] = nb / nc, err.sum(1) / nb                    # (0 / 0 = NaN: no such beat)
        tc, tb = float(nc[keep].sum()), float(nb[keep].sum())
        pooled[key + "_share"] = tb / tc if tc else float("nan")
        pooled[key + "_mae_ms"] = float(err[keep].sum()) / tb if tb else float("nan")
        pooled[key + "_beats"] = int(tb)
    return share, mae, pooled


def evaluate_intervals(denoiser, records, noise, snr_db, ref=None, offsets=None, rng=None, delineator=None, detector=None):
    """The noise-stress protocol scored in intervals: `mix_records(records, noise, snr_db, offsets, rng)`,
    `denoiser.denoise(noisy)`, then the clean, the noisy and the denoised records are delineated AT THE SAME BEATS `ref` (`Beats`
    or per-record lists; default: the detections on the clean records), and per condition and per record the share of the beats
    measurable in the clean record that are measurable here too, and the mean absolute error of QRS duration and of QT over the
    beats measurable in both, are taken -> `IntervalEvaluation`.  `denoiser` is a `StreamingDenoiser`, a `RateStreamingDenoiser`
    or a `ClassicalDenoiser`; delineator and detector (defaults `BeatDelineator(fs)`, `BeatDetector(fs)`) run at that object's
    outer rate `fs`, 360 Hz where it names none."""
    fs, dev, clean, noisy, out = stress_front(denoiser, records, noise, snr_db, offsets, rng)
    dl = delineator or BeatDelineator(fs, device=dev)
    if ref is None:
        ref = (detector or BeatDetector(fs, device=dev)).detect(clean)
    f_clean = dl.delineate(clean, ref)
    ref = Beats(f_clean.peaks, f_clean.count, fs)            # (lists are uploaded once)
    f_noisy, f_out = dl.delineate(noisy, ref), dl.delineate(out, ref)
    share, mae, pooled = {}, {}, {}
    for key, f in (("noisy", f_noisy), ("denoised", f_out)):
        share[key], mae[key], pooled[key] = interval_scores(f_clean, f)
    return IntervalEvaluation(f_clean, f_noisy, f_out, ref, share, mae, pooled)
