"""Median beats on the device: the representative beat of every window of a record, and the intervals a reader takes from it.

    tpl = MedianBeat(fs=360).average(records, beats, classes)      # whole records, ral_template_records -> BeatTemplates
    tpl.delineate(), tpl.intervals()                               # the template's fiducial points, QRS / QT / QTc per window
    tpl.pst()                                                      # its P wave and ST level (`PStMeasurer`)
    ev = evaluate_templates(denoiser, records, noise, snr_db)      # the noise-stress protocol: is the shape of the beat back?

The definition (include/ralenet.h has the same one).  Input (R, leads, T) fp32 at rate fs and, per record, strictly ascending
beat positions p_0 < ... < p_{n-1} in [0, T) - a `Beats`, or per-record lists - and optionally labels l_i (a `BeatClasses`, or
per-record lists); without labels every beat is N.  Geometry (`template_geometry`; exact rational arithmetic, round = nearest,
halves up):

    Wpre = round(0.35 fs) = 126 at 360 Hz, 175 at 500 Hz;  Wpost = round(0.65 fs) = 234, 325;  Wn = Wpre + Wpost + 1 = 361, 501
    W = round(win_s fs), H = round(hop_s fs)      window and hop in samples (10 s, 10 s);  KMAX = 256

Windows of a record of length T, the rule of `hrv_windows`: nw = max(1, (T - W) // H + 1), window w = [w H, min(w H + W, T)).
Beat i is a member of window w iff w0 <= p_i < w1, l_i == 0 when labels are given, and p_i - Wpre >= 0 and p_i + Wpost <= T - 1: a
beat whose samples leave the record is not used, there is no clamping.  `total` is the number of members; the first
used = min(total, KMAX) of them, in list order, are measured.

    tpl[l][k]   the median over the used beats of x_l[p_j - Wpre + k], k = 0 .. Wn - 1: the middle value of an odd count,
                (a + b) * 0.5f of the two middle values of an even count - one fp32 addition and then one product, so nothing
                can contract into an FMA; used == 0: all zeros
    rr          over the used beats whose index in the record's list is i >= 1, the lower median sorted[(m - 1) // 2] of the
                integers p_i - p_{i-1} (the previous beat of the list, whatever its label or window); -1 where there are none

Non-finite samples are out of scope, as elsewhere.  The results are reproducible bit for bit and do not depend on the launch
geometry; the sign of a zero median is unspecified.

Device tensors only: there is no CPU fallback."""
import torch

from . import _lib
from .beats import MODEL_RATE, BeatDetector, Beats, _round
from .delineate import BeatDelineator, Fiducials, interval_scores
from .evaluate import stress_front
from .hrv import _labels, _sec, hrv_windows
from .intake import beat_lists, check_leads, device_records, record_shape
from .model import _ptr, _stream
from .pst import PStMeasurer, PStPoints
from .rate import _rate
from .rhythm import BeatClassifier

KMAX = 256
_MAX_HALF = 2 ** 19               # ral_template.hip: Wpre, Wpost <= 2^19, so that the tiles of a template fit a grid dimension
_MAX_RECORDS = 65535              # records per call, of ral_template_records and of ral_delineate_records


def template_geometry(fs=MODEL_RATE, win_s=10, hop_s=10):
    """-> {fs, Wpre, Wpost, Wn, W, H, KMAX} in samples at rate `fs` (a positive int or Fraction); nothing is refused here
    (`template_check`)"""
    fs = _rate(fs, "fs")
    win, hop = _sec(win_s, "win_s"), _sec(hop_s, "hop_s")
    pre, post = _round(fs * 7 / 20), _round(fs * 13 / 20)
    return {"fs": fs, "Wpre": int(pre), "Wpost": int(post), "Wn": int(pre + post + 1), "W": int(_round(win * fs)),
            "H": int(_round(hop * fs)), "KMAX": KMAX}


def template_check(g, leads):
    """raise RalError, naming the broken rule, unless the geometry and the leads are ones ral_template_records supports -> the
    geometry"""
    check_leads(leads, "median beat", 65535)
    rules = (("1 <= Wpre <= 2^19", 1 <= g["Wpre"] <= _MAX_HALF), ("1 <= Wpost <= 2^19", 1 <= g["Wpost"] <= _MAX_HALF),
             ("1 <= W < 2^31", 1 <= g["W"] < 2 ** 31), ("1 <= H < 2^31", 1 <= g["H"] < 2 ** 31),
             ("1 <= KMAX <= 256", 1 <= g["KMAX"] <= KMAX))
    for rule, ok in rules:
        if not ok:
            raise _lib.RalError(f"median beat: this geometry is not supported: need {rule} (Wpre={g['Wpre']} Wpost={g['Wpost']} "
                                f"W={g['W']} H={g['H']} KMAX={g['KMAX']} at fs={g['fs']})")
    return g


def _classes(classes, peaks, count, what):
    """the labels as `HrvAnalyzer.analyse` takes them - a `BeatClasses`, per-record lists or None - or, already on the device, an
    (R, cap) int32 tensor aligned with `peaks` -> (R, cap) int32 on the device of `peaks`, or None"""
    if torch.is_tensor(classes) and classes.dim() == 2:
        if classes.shape != peaks.shape or classes.device != peaks.device or classes.dtype != torch.int32:
            raise _lib.RalError(f"{what}: labels of shape {tuple(classes.shape)} ({classes.dtype}) on {classes.device} for beats "
                                f"of shape {tuple(peaks.shape)} on {peaks.device}")
        return classes.contiguous()
    return _labels(classes, peaks, count, what)


class BeatTemplates:
    """What `MedianBeat.average` returns: `template` (R, nw, leads, Wn) fp32, the median beat of every window of every record
    (zeros where `used` is 0); `used`, `total`, `rr` (R, nw) int32, how many beats the template was taken over, how many members
    the window has, and the lower median of their RR intervals in samples (-1: none), all on the device; `index` (nw, 2) int64
    on the host, the windows [w0, w1); `center` = Wpre, the sample of a template where its beats' positions lie; `fs`,
    `geometry`.  len() is R."""

    def __init__(self, template, used, total, rr, index, fs, geometry):
        self.template, self.used, self.total, self.rr, self.index = template, used, total, rr, index
        self.fs, self.geometry, self.center = fs, geometry, geometry["Wpre"]

    def __len__(self):
        return self.template.shape[0]

    @torch.no_grad()
    def delineate(self, delineator=None, min_beats=3):
        """-> the `Fiducials` of the templates, measured by `BeatDelineator` (default `BeatDelineator(fs)`) as R * nw records
        `template.view(R * nw, leads, Wn)` with one beat each at `center` where `used >= min_beats` and none elsewhere: on,
        off, tpeak, tend (R * nw, 1), indices relative to the template"""
        R, nw, leads, Wn = self.template.shape
        dev = self.template.device
        dl = delineator or BeatDelineator(self.fs, device=dev)
        x = self.template.view(R * nw, leads, Wn)
        peaks = torch.full((R * nw, 1), self.center, dtype=torch.int32, device=dev)
        count = (self.used.reshape(-1) >= int(min_beats)).to(torch.int32)
        parts = [dl.delineate(x[a:a + _MAX_RECORDS], Beats(peaks[a:a + _MAX_RECORDS], count[a:a + _MAX_RECORDS], self.fs))
                 for a in range(0, R * nw, _MAX_RECORDS)]
        if len(parts) == 1:
            return parts[0]
        return Fiducials(*(torch.cat([getattr(f, k) for f in parts]) for k in ("on", "off", "tpeak", "tend")), peaks, count, self.fs)

    @torch.no_grad()
    def pst(self, measurer=None, delineator=None, min_beats=3):
        """-> the `PStPoints` of the templates, measured by `PStMeasurer` (default `PStMeasurer(fs)`) on the records and the
        `Fiducials` of `delineate(delineator, min_beats)`: pon, ppeak, poff (R * nw, 1) and st (R * nw, 1, leads), indices
        relative to the template.  A template's beat has no neighbour, so its P search is [on - Wp, on - g]."""
        R, nw, leads, Wn = self.template.shape
        ms = measurer or PStMeasurer(self.fs, device=self.template.device)
        f = self.delineate(delineator, min_beats)
        x = self.template.view(R * nw, leads, Wn)
        keys = ("on", "off", "tpeak", "tend", "peaks", "count")
        parts = [ms.measure(x[a:a + _MAX_RECORDS], Fiducials(*(getattr(f, k)[a:a + _MAX_RECORDS] for k in keys), f.fs))
                 for a in range(0, R * nw, _MAX_RECORDS)]
        if len(parts) == 1:
            return parts[0]
        return PStPoints(*(torch.cat([getattr(p, k) for p in parts]) for k in ("pon", "ppeak", "poff", "st")), f.on, f.peaks,
                         f.count, self.fs)

    @torch.no_grad()
    def intervals(self, delineator=None, min_beats=3):
        """-> {"qrs_ms", "qt_ms", "qtc_ms"}, each (R, nw) fp32, NaN where a point is missing: the formulas of `Fiducials` on the
        template's points, formed in fp64 and rounded once; Bazett's correction divides by the square root of `rr / fs`
        seconds and is NaN where `rr` < 0"""
        f = self.delineate(delineator, min_beats)
        shape = tuple(self.used.shape)
        rr = self.rr.reshape(-1, 1)
        rr_s = torch.where(rr >= 0, rr.double() / float(self.fs), torch.full(rr.shape, float("nan"), dtype=torch.float64, device=rr.device))
        qrs, qt = f._ms64(f.on, f.off), f._ms64(f.on, f.tend)
        return {"qrs_ms": qrs.float().view(shape), "qt_ms": qt.float().view(shape), "qtc_ms": (qt / torch.sqrt(rr_s)).float().view(shape)}


class MedianBeat:
    """Median beats of whole records at rate `fs` (`ral_template_records`).  `average(records, beats, classes=None)` takes a
    device tensor (leads, T) or (R, leads, T), the beats of every record - a `Beats`, or per-record lists of strictly ascending
    positions in [0, T), which are checked on the host - and their labels - a `BeatClasses`, per-record lists, an (R, cap) int32
    device tensor aligned with the beats, or None: every beat is N - and returns `BeatTemplates`."""

    def __init__(self, fs=MODEL_RATE, win_s=10, hop_s=10, device="cuda"):
        self.fs, self.geometry = fs, template_geometry(fs, win_s, hop_s)
        g = self.geometry
        self.geom = _lib.TemplateGeom(*(min(g[k], 2 ** 31 - 1) for k in ("Wpre", "Wpost", "W", "H", "KMAX")))
        self.device = torch.device(device)

    @torch.no_grad()
    def average(self, records, beats, classes=None):
        what = "MedianBeat.average"
        R, leads, T = record_shape(records, what)
        g = template_check(self.geometry, leads)
        peaks, count = beat_lists(beats, records.device, what, T=T, R=R)       # (the lists are checked on the host)
        label = _classes(classes, peaks, count, what)
        x = device_records(records, what)
        win = hrv_windows(T, g)
        cap, nw = peaks.shape[1], len(win)
        with torch.cuda.device(x.device):
            tpl = torch.empty(R, nw, leads, g["Wn"], dtype=torch.float32, device=x.device)
            used, total, rr = (torch.empty(R, nw, dtype=torch.int32, device=x.device) for _ in range(3))
            _lib.check(_lib.lib().ral_template_records(_ptr(x), R, leads, T, self.geom, _ptr(peaks),
                                                       None if label is None else _ptr(label), _ptr(count), cap, nw, _ptr(tpl),
                                                       _ptr(used), _ptr(total), _ptr(rr), _stream()))
        return BeatTemplates(tpl, used, total, rr, win, self.fs, g)


class TemplateEvaluation:
    """What `evaluate_templates` returns: `clean`, `noisy`, `denoised`, the `BeatTemplates` of the three records at the same
    beats `ref` and labels `labels` ((R, cap) int32 on the device); `rmse` = {"noisy": (R, nw) fp64, "denoised": ...}, per window
    the root mean square over leads and samples of the template's difference from the clean one, NaN where the window has
    fewer than `min_beats` used beats; `pooled_rmse` = {"noisy", "denoised"}, the same over all such windows as plain numbers
    (NaN where there is none) and `windows` how many there are; `fiducials` = {"clean", "noisy", "denoised"}, the `Fiducials` of
    the templates; `share`, `mae_ms`, `pooled` as in `IntervalEvaluation` (`interval_scores` on those), a template in the place of
    a record: `share[key][name]` and `mae_ms[key][name]` are (R, nw)."""

    def __init__(self, clean, noisy, denoised, ref, labels, rmse, pooled_rmse, windows, fiducials, share, mae_ms, pooled):
        self.clean, self.noisy, self.denoised, self.ref, self.labels = clean, noisy, denoised, ref, labels
        self.rmse, self.pooled_rmse, self.windows, self.fiducials = rmse, pooled_rmse, windows, fiducials
        self.share, self.mae_ms, self.pooled = share, mae_ms, pooled


def template_rmse(clean, other, min_beats=3):
    """two `BeatTemplates` of the same beats -> ((R, nw) fp64 RMSE of `other` against `clean` over leads and samples, NaN where
    `clean.used < min_beats`; the same over all other windows as a plain number, NaN where there is none; how many there are)"""
    ok = clean.used >= int(min_beats)
    se = (other.template.double() - clean.template.double()).pow(2).sum((2, 3))
    per = clean.template.shape[2] * clean.template.shape[3]
    nan = torch.full(se.shape, float("nan"), dtype=torch.float64, device=se.device)
    n = int(ok.sum())
    return torch.where(ok, torch.sqrt(se / per), nan), float(torch.sqrt(se[ok].sum() / (n * per))) if n else float("nan"), n


def evaluate_templates(denoiser, records, noise, snr_db, ref=None, ref_labels=None, offsets=None, rng=None, averager=None,
                       delineator=None, detector=None, classifier=None, min_beats=3):
    """The noise-stress protocol scored in the shape of the beat: `mix_records(records, noise, snr_db, offsets, rng)`,
    `denoiser.denoise(noisy)`, then the median beats of the clean, the noisy and the denoised records are taken AT THE SAME
    BEATS `ref` (`Beats` or per-record lists; default: the detections on the clean records) AND LABELS `ref_labels` (a
    `BeatClasses` or per-record lists; default: the classes of `ref` in the clean records), and per window the RMSE of the noisy
    and of the denoised template against the clean one, and `interval_scores` of the templates' `Fiducials`, are taken ->
    `TemplateEvaluation`.  averager, delineator, detector and classifier (defaults `MedianBeat(fs)`, `BeatDelineator(fs)`,
    `BeatDetector(fs)`, `BeatClassifier(fs)`) run at the denoiser's outer rate `fs`, 360 Hz where it names none."""
    fs, dev, clean, noisy, out = stress_front(denoiser, records, noise, snr_db, offsets, rng)
    avg = averager or MedianBeat(fs, device=dev)
    dl = delineator or BeatDelineator(fs, device=dev)
    if ref is None:
        ref = (detector or BeatDetector(fs, device=dev)).detect(clean)
    peaks, count = beat_lists(ref, dev, "evaluate_templates", T=clean.shape[-1], R=clean.shape[0])
    ref = Beats(peaks, count, fs)                            # (lists are uploaded once)
    if ref_labels is None:
        ref_labels = (classifier or BeatClassifier(fs, device=dev)).classify(clean, ref)
    labels = _classes(ref_labels, peaks, count, "evaluate_templates")
    t_clean, t_noisy, t_out = (avg.average(x, ref, labels) for x in (clean, noisy, out))
    fid = {k: t.delineate(dl, min_beats) for k, t in (("clean", t_clean), ("noisy", t_noisy), ("denoised", t_out))}
    rmse, pooled_rmse, share, mae, pooled, windows = {}, {}, {}, {}, {}, 0
    shape = tuple(t_clean.used.shape)
    for key, t in (("noisy", t_noisy), ("denoised", t_out)):
        rmse[key], pooled_rmse[key], windows = template_rmse(t_clean, t, min_beats)
        s, m, pooled[key] = interval_scores(fid["clean"], fid[key])
        share[key], mae[key] = {k: v.view(shape) for k, v in s.items()}, {k: v.view(shape) for k, v in m.items()}
    return TemplateEvaluation(t_clean, t_noisy, t_out, ref, labels, rmse, pooled_rmse, windows, fid, share, mae, pooled)
