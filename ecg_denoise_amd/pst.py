"""P wave and ST level on the device: where does the P wave of a delineated beat begin, peak and end, and how far does the ST
segment lie from the isoelectric level?

    fid = BeatDelineator(fs=360).delineate(records, beats)         # the QRS onset and offset of every beat
    pst = PStMeasurer(fs=360).measure(records, fid)                # whole records, ral_pst_records -> PStPoints
    pst.pr_ms(), pst.p_ms(), pst.st                                # PR interval, P duration, ST level per lead
    ev = evaluate_pst(denoiser, records, noise, snr_db)            # the noise-stress protocol scored in P waves, PR and ST

The measurement (include/ralenet.h has the same definition).  Input (R, leads, T) fp32 at rate fs, per record strictly ascending
beat positions p_0 < ... < p_{n-1} in [0, T), and per beat the delineator's `on` and `off`: a `Fiducials`.  c(t) = clamp(t, 0,
T - 1).  Lengths in samples (`pst_geometry`; the rounding of `delineate_geometry`: nearest, halves up, exact):

    m2 = round(fs / 60) = 6 at 360 Hz (the delineator's smoothed leads z_l[t] = sum_{k = -m2 .. m2} x_l[c(t + k)], k ascending);
    g = round(fs / 50) = 7 (the delineator's quiet-run length);  Wp = round(0.30 fs) = 108 (how far before the onset a P wave
    is searched);  j = round(0.06 fs) = 22 (ST is read at J + 60 ms, J = off)

All floating arithmetic is fp32, every sum is taken one term at a time in the order written, and no product is ever followed by
an addition, so nothing can contract into an FMA: the three integers and the ST levels of a beat are reproducible bit for bit.

Validity: the `on` of the beat at p counts only if 0 <= on <= p, its `off` only if p <= off <= T - 1; anything else, -1 included,
is "missing".  The kernel decides this itself, so that no read can leave the record whatever the tensors hold.

    isoelectric level (needs on)   e = max(on - g, 0) and b_l = z_l[e]: by the definition of on, e lies in the quiet run in front
                                   of the QRS, which is the PR segment
    deviation                      s[t] = sum_l |z_l[t] - b_l|, in lead order

ST level (needs on and off): ts = off + j; lim = T - 1, and when beat i + 1 exists lim is also capped at p + (2 (p_{i+1} - p)) // 3.
ts <= lim: st_l = (z_l[ts] - b_l) * w per lead, one subtraction and one product, with w = fp32(1 / (2 m2 + 1)) formed on the host:
the unit is that of the samples.  Otherwise st_l = NaN.

P wave (needs on): phi = e; plo = max(on - Wp, 0), and when beat i - 1 exists plo is also at least p_{i-1} + (2 (p - p_{i-1})) // 3:
the P search gets the last third of the interval, the previous beat's T search ends where it starts.  plo > phi: no P.

    S        max s[t] over [on, max(off, p)], p in the place of a missing off: the QRS on the same scale
    ppeak    the first argmax of s over [plo, phi]; no P if ppeak == plo, or ppeak == phi, or s[ppeak] == 0, or
             s[ppeak] < p0 * S, one fp32 product (default p0 = 0.08): an argmax on the edge is the previous T wave's tail or the
             Q wave, not a P wave
    pon      the first argmax over t in [plo, ppeak] of (s[ppeak] - s[t]) * float(t + ppeak - 2 plo)
    poff     the first argmax over t in [ppeak, phi] of (s[ppeak] - s[t]) * float(2 phi - ppeak - t): the trapezium rule of
             tend, mirrored for the onset
    no P     pon = ppeak = poff = -1

Every beat is measured on its own, by one wave: its result depends only on the record, its own position, on and off, and the
positions of the two neighbouring beats.

Non-finite samples are out of scope, as for the delineator.  The default p0 was chosen on synthetic data (`synth`) only; it has
not been tuned on a database.

Device tensors only: there is no CPU fallback."""
import numpy as np
import torch

from . import _lib
from .beats import MODEL_RATE, BeatDetector, Beats, _round
from .delineate import BeatDelineator, Fiducials
from .evaluate import stress_front
from .intake import beat_lists, check_leads, device_records, record_shape
from .model import _ptr, _stream
from .rate import _rate

# the LDS budget of ral_pst.hip (pst_geom there): a wave keeps s over [plo, phi], at most Wp + 1 floats, and the samples of one
# lead under it, at most Wp + 2 m2 + 1
_LDS_BYTES = 65536


def pst_geometry(fs=MODEL_RATE):
    """-> {m2, g, Wp, j} in samples at rate `fs` (a positive int or Fraction)"""
    fs = _rate(fs, "fs")
    return {"m2": _round(fs / 60), "g": _round(fs / 50), "Wp": _round(fs * 3 / 10), "j": _round(fs * 3 / 50)}


def pst_check(fs, leads):
    """raise RalError unless the P window at rate `fs` fits the kernel's LDS budget -> the geometry"""
    g = pst_geometry(fs)
    check_leads(leads, "P and ST measurement", 65535)
    if g["g"] < 1 or g["Wp"] < 1 or 4 * (2 * g["Wp"] + 2 * g["m2"] + 2) > _LDS_BYTES:
        raise _lib.RalError(f"P and ST measurement at fs={fs} is not supported: the P window of one beat ({g['Wp'] + 1} and "
                            f"{g['Wp'] + 2 * g['m2'] + 1} samples) does not fit the kernel's {_LDS_BYTES // 1024} KB of LDS")
    return g


class PStPoints:
    """What `PStMeasurer.measure` returns: `pon`, `ppeak`, `poff` (R, cap) int32 on the device, the onset, the peak and the end
    of every beat's P wave as sample indices, -1 where the beat has no P wave and in the padding; `st` (R, cap, leads) fp32, the
    ST level of every lead in the unit of the samples, NaN where it cannot be read and in the padding; `on` and `peaks` (R, cap)
    int32 are the QRS onsets and the positions that were measured, `count` (R,) int32 how many beats each record has, `fs` the
    rate the indices refer to.  The intervals are torch operations on these tensors: (R, cap) fp32, NaN where a point is
    missing."""

    def __init__(self, pon, ppeak, poff, st, on, peaks, count, fs=MODEL_RATE):
        self.pon, self.ppeak, self.poff, self.st, self.on, self.peaks, self.count, self.fs = pon, ppeak, poff, st, on, peaks, count, fs

    def __len__(self):
        return self.pon.shape[0]

    def tolist(self):
        """-> [(pon, ppeak, poff, st) of record r: three plain lists of count[r] values and one of count[r] lists of `leads`
        values] (synchronises)"""
        n = self.count.tolist()
        cols = [t.tolist() for t in (self.pon, self.ppeak, self.poff, self.st)]
        return [tuple(c[r][:k] for c in cols) for r, k in enumerate(n)]

    def _ms64(self, a, b):
        """(b - a) 1000 / fs in fp64, NaN where either point is missing"""
        nan = torch.full(a.shape, float("nan"), dtype=torch.float64, device=a.device)
        return torch.where((a >= 0) & (b >= 0), (b - a).double() * 1000.0 / float(self.fs), nan)

    def pr_ms(self):
        """PR interval (on - pon) 1000 / fs in ms (formed in fp64, rounded once)"""
        return self._ms64(self.pon, self.on).float()

    def p_ms(self):
        """P duration (poff - pon) 1000 / fs in ms (formed in fp64, rounded once)"""
        return self._ms64(self.pon, self.poff).float()

    def measurable(self):
        """-> {"p": (R, cap) bool, a P wave was found; "st": (R, cap) bool, the ST level was read (of every lead, or of none)}"""
        return {"p": self.ppeak >= 0, "st": ~torch.isnan(self.st[..., 0])}


class PStMeasurer:
    """P onset, peak and end and the ST level per lead of the delineated beats of whole records at rate `fs`
    (`ral_pst_records`).  `measure(records, fiducials)` takes a device tensor (leads, T) or (R, leads, T) and the `Fiducials`
    that `BeatDelineator.delineate` gave for these records, of which `peaks`, `count`, `on` and `off` are used, and returns
    `PStPoints`."""

    def __init__(self, fs=MODEL_RATE, p0=0.08, device="cuda"):
        self.fs, self.p0, self.geometry = fs, float(p0), pst_geometry(fs)
        if not (np.isfinite(self.p0) and self.p0 >= 0):
            raise _lib.RalError(f"PStMeasurer.measure: need a finite p0 >= 0 (got p0={p0!r})")
        g = self.geometry
        self.geom = _lib.PstGeom(g["m2"], g["g"], g["Wp"], g["j"], 1.0 / (2 * g["m2"] + 1), self.p0)
        self.device = torch.device(device)

    @torch.no_grad()
    def measure(self, records, fiducials):
        what = "PStMeasurer.measure"
        R, leads, T = record_shape(records, what)
        pst_check(self.fs, leads)
        f = fiducials
        if not isinstance(f, Fiducials):
            raise _lib.RalError(f"{what}: expected the Fiducials of BeatDelineator.delineate, got {type(f).__name__}")
        peaks, count = beat_lists(Beats(f.peaks, f.count, f.fs), records.device, what, T=T, R=R)
        if f.fs != self.fs:
            raise _lib.RalError(f"{what}: fiducials at fs={f.fs} for a measurement at fs={self.fs}")
        for name, t in (("on", f.on), ("off", f.off)):       # (a cap that is not that of the positions)
            if t.shape != peaks.shape or t.dtype != torch.int32 or t.device != peaks.device:
                raise _lib.RalError(f"{what}: fiducials whose `{name}` is {tuple(t.shape)} {t.dtype} on {t.device} for positions "
                                    f"{tuple(peaks.shape)} {peaks.dtype} on {peaks.device}")
        x = device_records(records, what)
        on, off = f.on.contiguous(), f.off.contiguous()
        cap = peaks.shape[1]
        with torch.cuda.device(x.device):
            pon, ppeak, poff = (torch.empty(R, cap, dtype=torch.int32, device=x.device) for _ in range(3))
            st = torch.empty(R, cap, leads, dtype=torch.float32, device=x.device)
            _lib.check(_lib.lib().ral_pst_records(_ptr(x), R, leads, T, self.geom, _ptr(peaks), _ptr(count), cap, _ptr(on),
                                                  _ptr(off), _ptr(pon), _ptr(ppeak), _ptr(poff), _ptr(st), _stream()))
        return PStPoints(pon, ppeak, poff, st, on, peaks, count, self.fs)


class PStEvaluation:
    """What `evaluate_pst` returns: `clean`, `noisy`, `denoised`, the `PStPoints` of the three records at the same beats `ref`,
    and `fiducials` = {"clean", "noisy", "denoised"}, the `Fiducials` they were measured from; `share` = {"noisy": {"p": (R,)},
    "denoised": {...}}, per record the share of the clean record's P waves that are found here too; `mae` = {"noisy": {"pr_ms":
    (R,), "st": (R, leads)}, "denoised": {...}}, per record the mean absolute error of the PR interval in ms over the beats that
    have a P wave in both, and per record and lead that of the ST level over the beats that have one in both (fp64 on the
    device, NaN where there is no such beat); `pooled` = {"noisy": {"p_share", "pr_mae_ms", "p_beats", "st_mae", "st_beats"},
    "denoised": {...}}, the same over the beats of all records as plain numbers (`st_mae`: one per lead; `*_beats`: how many
    beats had the value in both).  The ST errors are in the unit of the mixed records, which `mix_records` z-scores: standard
    deviations of the clean lead, not millivolts."""

    def __init__(self, clean, noisy, denoised, ref, fiducials, share, mae, pooled):
        self.clean, self.noisy, self.denoised, self.ref, self.fiducials = clean, noisy, denoised, ref, fiducials
        self.share, self.mae, self.pooled = share, mae, pooled


def pst_scores(clean, other, rows=None):
    """the `PStPoints` of the clean records and of another condition at the same beats -> (share, mae, pooled) as in
    `PStEvaluation`; `rows` (a bool or index tensor over the records) narrows the pooled values"""
    mc, mo = clean.measurable(), other.measurable()
    keep = torch.ones(len(clean), dtype=torch.bool, device=clean.pon.device)
    if rows is not None:
        keep = torch.zeros_like(keep)
        keep[rows] = True
    zero = torch.zeros((), dtype=torch.float64, device=keep.device)
    both = mc["p"] & mo["p"]
    err = torch.where(both, (other.pr_ms().double() - clean.pr_ms().double()).abs(), zero)
    nc, nb = mc["p"].sum(1).double(), both.sum(1).double()
    share, mae = {"p": nb / nc}, {"pr_ms": err.sum(1) / nb}                  # (0 / 0 = NaN: no such beat)
    tc, tb = float(nc[keep].sum()), float(nb[keep].sum())
    pooled = {"p_share": tb / tc if tc else float("nan"), "pr_mae_ms": float(err[keep].sum()) / tb if tb else float("nan"),
              "p_beats": int(tb)}
    both = mc["st"] & mo["st"]
    err = torch.where(both[..., None], (other.st.double() - clean.st.double()).abs(), zero)
    nb = both.sum(1).double()
    mae["st"] = err.sum(1) / nb[:, None]
    tb = float(nb[keep].sum())
    leads = clean.st.shape[2]
    pooled["st_mae"] = (err[keep].sum((0, 1)) / tb).tolist() if tb else [float("nan")] * leads
    pooled["st_beats"] = int(tb)
    return share, mae, pooled


def evaluate_pst(denoiser, records, noise, snr_db, ref=None, offsets=None, rng=None, measurer=None, delineator=None, detector=None):
    """The noise-stress protocol scored in the P wave and the ST level: `mix_records(records, noise, snr_db, offsets, rng)`,
    `denoiser.denoise(noisy)`, then the clean, the noisy and the denoised records are delineated AT THE SAME BEATS `ref` (`Beats`
    or per-record lists; default: the detections on the clean records) and measured, and per condition, per record and pooled,
    the share of the clean record's P waves that are still found, the mean absolute error of the PR interval in ms over the
    beats that have a P wave in both, and that of the ST level per lead over the beats that have one in both, are taken ->
    `PStEvaluation`.  The ST errors are in the unit of the mixed records, which `mix_records` z-scores.  `denoiser` is a
    `StreamingDenoiser`, a `RateStreamingDenoiser` or a `ClassicalDenoiser`; measurer, delineator and detector (defaults
    `PStMeasurer(fs)`, `BeatDelineator(fs)`, `BeatDetector(fs)`) run at that object's outer rate `fs`, 360 Hz where it names
    none."""
    fs, dev, clean, noisy, out = stress_front(denoiser, records, noise, snr_db, offsets, rng)
    ms = measurer or PStMeasurer(fs, device=dev)
    dl = delineator or BeatDelineator(fs, device=dev)
    if ref is None:
        ref = (detector or BeatDetector(fs, device=dev)).detect(clean)
    f_clean = dl.delineate(clean, ref)
    ref = Beats(f_clean.peaks, f_clean.count, fs)            # (lists are uploaded once)
    fid = {"clean": f_clean, "noisy": dl.delineate(noisy, ref), "denoised": dl.delineate(out, ref)}
    pts = {k: ms.measure(x, fid[k]) for k, x in (("clean", clean), ("noisy", noisy), ("denoised", out))}
    share, mae, pooled = {}, {}, {}
    for key in ("noisy", "denoised"):
        share[key], mae[key], pooled[key] = pst_scores(pts["clean"], pts[key])
    return PStEvaluation(pts["clean"], pts["noisy"], pts["denoised"], ref, fid, share, mae, pooled)
