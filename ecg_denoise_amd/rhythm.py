"""Beat classes on the device: is a detected beat normal (N), ventricular (V) or premature with a normal shape (S)?

    classes = BeatClassifier(fs=360).classify(records, beats)      # whole records, ral_rhythm_records -> BeatClasses
    pool = BeatClassPool(leads, capacity, fs=360)                  # chunks of independent streams: BeatPool + ral_rhythm_pool
    ev = evaluate_rhythm(denoiser, records, noise, snr_db)         # the noise-stress protocol scored in beat classes

The classifier (include/ralenet.h has the same definition).  Input (R, leads, T) fp32 at rate fs and, per record, an ascending
list of beat positions p_0 < ... < p_{n-1} in [0, T): a `Beats` from `BeatDetector`, or per-record lists such as annotations.
Lengths in samples (`rhythm_geometry`; the rounding of `beat_geometry`: nearest, halves up, exact):

    Wb = round(0.1 fs) = 36 at 360 Hz;  Sa = round(fs / 120) = 3;  K = 8, min_ref = 3, c0 = 0.7, r0 = 0.8

For beat i of a record with n beats:

    neighbourhood  a = min(max(i - K, 0), max(0, n - K - 1)); the neighbours are the beats j in [a, min(n, a + K + 1)), j != i:
                   the eight beats before i for i >= K; the first eight beats of a record serve each other, with beat 8; a
                   record of n <= K beats uses all its other beats.  Fewer than min_ref neighbours: unclassified, label -1,
                   both features NaN.
    windows        w_j[l][k] = x_l[clamp(p_j + k, 0, T - 1)] for k = -Wb .. Wb, minus that window's own mean over k
    template       t[l][k] = median over the neighbours of w_j[l][k] (an even number: half the sum of the two middle values)
    correlation    for s in [-Sa, Sa]: v_s[l][k] = x_l[clamp(p_i + s + k, 0, T - 1)] minus its mean over k;
                   corr_s = sum_l sum_k t v_s / sqrt(sum t^2 * sum v_s^2), 0 where the denominator is 0; corr = max over s
    RR ratio       rr_ratio = (p_i - p_{i-1}) / median of the differences of consecutive positions among the beats
                   [a, min(n, a + K + 1)) (beat i among them); NaN for i = 0
    label          1 (V) iff corr < c0; otherwise 2 (S) iff i > 0 and rr_ratio < r0; otherwise 0 (N)
    logits         [corr - c0, c0 - corr] per classified beat, so argmax == 1 iff V: `scoring.acc / precision / f1_score`
                   apply as they are

Every beat is classified on its own, by one wave, in an order that depends on the geometry alone, so a stream classified
push by push gives exactly the bits of the complete record.  Beat i of a stream is final when beat max(i, K) has been given by
the detector or the stream has closed (its samples have always been received by then): the first eight beats of a stream come
out together with the ninth, or at close; after that every beat comes out in the push that detects it.

Non-finite samples are out of scope, as for the detector.  The defaults were chosen on synthetic data (`synth`) only; none has
been tuned on MIT-BIH.

Device tensors only: there is no CPU fallback."""
import numpy as np
import torch

from . import _lib, scoring
from .beats import MODEL_RATE, BeatDetector, BeatPool, BeatPoolState, Beats, _lag, _round
from .evaluate import stress_front
from .intake import beat_lists, check_leads, device_records, pad_rows, record_shape
from .model import _ptr, _stream
from .pools import StreamSurface, as_chunks, pack_chunks, scratch_bytes, table_buffer
from .rate import _rate

K, MIN_REF = _lib.RHYTHM_K, _lib.RHYTHM_MIN_REF
# the LDS budget of ral_rhythm.hip (rhythm_geom there): per lead a wave stages the windows of K neighbours, the template, the
# beat's own extended window, their means and the running sums, beside the sources and positions of the K + 1 beats
_LDS_BYTES, _NS_MAX = 65536, 56


def rhythm_geometry(fs=MODEL_RATE):
    """-> {Wb, Sa} in samples at rate `fs` (a positive int or Fraction)"""
    fs = _rate(fs, "fs")
    return {"Wb": _round(fs / 10), "Sa": _round(fs / 120)}


def _lds_bytes(g):
    W, We, NS = 2 * g["Wb"] + 1, 2 * (g["Wb"] + g["Sa"]) + 1, 2 * g["Sa"] + 1
    return (K + 1) * 32 + (2 * K + 1) * 8 + 4 * ((K + 1) * W + We + K + 3 * NS + 1)


def rhythm_check(fs, leads):
    """raise RalError unless the classifier's windows at rate `fs` fit the kernel's LDS budget -> the geometry"""
    g = rhythm_geometry(fs)
    check_leads(leads, "beat classes", 65535)
    if g["Wb"] < 1 or 2 * g["Sa"] + 1 > _NS_MAX or _lds_bytes(g) > _LDS_BYTES:
        raise _lib.RalError(f"beat classes at fs={fs} are not supported: the windows of {K} neighbours of one lead "
                            f"({2 * g['Wb'] + 1} samples each) and {2 * g['Sa'] + 1} shifts do not fit the kernel's "
                            f"{_LDS_BYTES // 1024} KB of LDS and {_NS_MAX} shifts")
    return g


def hood(i, n):
    """the neighbourhood of beat i of n -> (a, hi): the beats [a, hi), beat i among them"""
    a = min(max(i - K, 0), max(0, n - K - 1))
    return a, min(n, a + K + 1)


class BeatClasses:
    """What `BeatClassifier.classify` returns: `label` (R, cap) int32 (0 N, 1 V, 2 S, -1 unclassified or padding), `corr` and
    `rr_ratio` (R, cap) fp32 (NaN where unclassified or padding) and `count` (R,) int32, all on the device; `peaks` (R, cap)
    int32 are the positions that were classified, `c0` and `r0` the thresholds."""

    def __init__(self, label, corr, rr_ratio, count, peaks, c0, r0, fs=MODEL_RATE):
        self.label, self.corr, self.rr_ratio, self.count, self.peaks = label, corr, rr_ratio, count, peaks
        self.c0, self.r0, self.fs = float(c0), float(r0), fs

    def __len__(self):
        return self.label.shape[0]

    def tolist(self):
        """-> [(labels, corr, rr_ratio) of record r, three plain lists of count[r] values] (synchronises)"""
        n = self.count.tolist()
        return [(a[:k], b[:k], c[:k]) for a, b, c, k in zip(self.label.tolist(), self.corr.tolist(), self.rr_ratio.tolist(), n)]

    def classified(self):
        """-> (R, cap) bool: the beats that have a class"""
        return self.label >= 0

    def logits(self, mask=None):
        """-> ((m, 2) fp32 logits [corr - c0, c0 - corr] of the classified beats of all records in record order, the (R, cap)
        bool mask that selects them); `mask` narrows the selection (it is and-ed with `classified()`)"""
        sel = self.classified() if mask is None else self.classified() & mask
        d = self.corr[sel] - torch.tensor(self.c0, dtype=torch.float32, device=self.corr.device)
        return torch.stack([d, -d], dim=1), sel

    def counts(self):
        """-> (R, 4) int64 on the device: N, V, S and unclassified beats per record"""
        nvs = torch.stack([(self.label == c).sum(1) for c in (0, 1, 2)], dim=1)
        return torch.cat([nvs, self.count.long()[:, None] - nvs.sum(1, keepdim=True)], dim=1)


def _geom(g, c0, r0, what):
    c0, r0 = float(c0), float(r0)
    if not (np.isfinite(c0) and np.isfinite(r0)):
        raise _lib.RalError(f"{what}: need finite c0 and r0 (got c0={c0!r} r0={r0!r})")
    return _lib.RhythmGeom(g["Wb"], g["Sa"], c0, r0)


class BeatClassifier:
    """Beat classes of whole records at rate `fs` (`ral_rhythm_records`).  `classify(records, beats)` takes a device tensor
    (leads, T) or (R, leads, T) and the beats of every record - a `Beats`, or per-record lists of strictly ascending positions in
    [0, T), which are checked on the host - and returns `BeatClasses`."""

    def __init__(self, fs=MODEL_RATE, c0=0.7, r0=0.8, device="cuda"):
        self.fs, self.c0, self.r0, self.geometry = fs, float(c0), float(r0), rhythm_geometry(fs)
        self.geom = _geom(self.geometry, c0, r0, "BeatClassifier")
        self.device = torch.device(device)

    @torch.no_grad()
    def classify(self, records, beats):
        what = "BeatClassifier.classify"
        R, leads, T = record_shape(records, what)
        rhythm_check(self.fs, leads)
        peaks, count = beat_lists(beats, records.device, what, T=T, R=R)       # (the lists are checked on the host)
        x = device_records(records, what)
        cap = peaks.shape[1]
        with torch.cuda.device(x.device):
            label = torch.empty(R, cap, dtype=torch.int32, device=x.device)
            corr = torch.empty(R, cap, dtype=torch.float32, device=x.device)
            rr = torch.empty(R, cap, dtype=torch.float32, device=x.device)
            _lib.check(_lib.lib().ral_rhythm_records(_ptr(x), R, leads, T, self.geom, _ptr(peaks), _ptr(count), cap, _ptr(label),
                                                     _ptr(corr), _ptr(rr), _stream()))
        return BeatClasses(label, corr, rr, count, peaks, self.c0, self.r0, self.fs)


class RhythmPoolState:
    """The host side of a `BeatClassPool`, without a device: the detector pool's own state (`beats`, a `BeatPoolState`) and per
    slot how many beats its stream has had (`nb`) and how many of them have been given out (`done`: 0 while the first K wait,
    else `nb`).  `plan` checks the arguments of a call without changing anything; `table` builds the call's table
    (`_lib.RHYTHM_ROW`) once the detector has said how many new beats every stream has; `commit` applies it."""

    def __init__(self, leads, capacity, fs=MODEL_RATE, name="BeatClassPool", beats=None):
        self.geometry = rhythm_check(fs, leads)
        self.beats = BeatPoolState(leads, capacity, fs, name) if beats is None else beats
        g = self.beats.geometry
        if g["Rw"] + self.geometry["Wb"] + self.geometry["Sa"] > _lag(g):
            raise _lib.RalError(f"{name}: a beat's window (Rw + Wb + Sa samples past its decision) exceeds the detector's lag")
        self.fs, self.leads, self.capacity, self.name = fs, self.beats.leads, self.beats.capacity, name
        self.nb = np.zeros(self.capacity, dtype=np.int64)
        self.done = np.zeros(self.capacity, dtype=np.int64)

    def open(self):
        sid = self.beats.open()
        self.nb[sid] = self.done[sid] = 0
        return sid

    def plan(self, shapes, close=()):
        """-> (sids in row order, the detector's table); raises RalError for a bad argument"""
        return self.beats.plan(shapes, close)

    def table(self, btab, m):
        """the detector's table of a call and the new beats of every row -> the classifier's table"""
        m = np.asarray(m, dtype=np.int64)
        if m.shape != btab.shape or np.any(m < 0) or np.any(m > 0x7fffffff):
            raise _lib.RalError(f"{self.name}: one count of new beats per row, in [0, 2^31)")
        slot = btab["slot"].astype(np.int64)
        nb, done = self.nb[slot], self.done[slot]
        n = nb + m
        ends = btab["T"] >= 0
        ne = np.where(ends | (n >= K + 1), n - done, 0)
        tab = np.zeros(len(btab), dtype=_lib.RHYTHM_ROW)
        for f in ("n0", "T", "x_off", "slot", "c", "turn", "flags"):
            tab[f] = btab[f]
        tab["nb"], tab["e0"], tab["m"], tab["ne"] = nb, done, m, ne
        tab["new_off"], tab["out_off"] = np.cumsum(m) - m, np.cumsum(ne) - ne
        return tab

    def commit(self, tab):
        slot = tab["slot"]
        self.nb[slot] = tab["nb"] + tab["m"]
        self.done[slot] = np.where(tab["ne"] > 0, tab["e0"] + tab["ne"], tab["e0"])


class BeatClassPool(StreamSurface):
    """Beat classes of up to `capacity` independent live streams of `leads` leads at rate `fs`, chunk by chunk: it owns a
    `BeatPool` (`beats`) and classifies what that detects (`ral_rhythm_pool`).  `open()` returns a stream id;
    `push(chunks, close=())` takes {sid: (leads, c)} (c >= 0, host or device) for any subset of the open streams, ends the streams
    listed in `close`, and returns {sid: (peaks int64, label int32, corr fp32, rr_ratio fp32)} on the device for every sid named:
    the beats that became final with this call.  The first eight beats of a stream come out together with the ninth, or at
    close; after that every beat comes out in the push that detects it.  Concatenated per stream from `open` to `close`, the
    results equal `BeatClassifier.classify(record, BeatDetector.detect(record))` bit for bit, whatever the chunking and the
    other streams.  `close(sid, x=None)` ends one stream.  Every argument is checked on the host before any device work
    (`plan`); a call that raises has changed nothing.  Per slot the device keeps the positions and extended windows
    (2 (Wb + Sa) + 1 samples per lead) of the last K beats; the samples of a new beat's window are read from the history plane
    of the `BeatPool` that was current before the push, and from the chunk.  `push` synchronises (as `BeatPool.push` does)."""

    def __init__(self, leads, capacity, fs=MODEL_RATE, c0=0.7, r0=0.8, alpha=0.35, floor=0.0, band=(8, 24), device="cuda"):
        name = type(self).__name__
        self.geom = _geom(rhythm_check(fs, leads), c0, r0, name)
        self.beats = BeatPool(leads, capacity, fs, alpha, floor, band, device)
        self.state = RhythmPoolState(leads, capacity, fs, name, beats=self.beats.state)
        self.fs, self.leads, self.capacity, self.device = fs, self.beats.leads, self.beats.capacity, self.beats.device
        self.geometry, self.c0, self.r0 = self.state.geometry, float(c0), float(r0)
        we = 2 * (self.geometry["Wb"] + self.geometry["Sa"]) + 1
        self.ring = torch.zeros(self.capacity, K, self.leads, we, dtype=torch.float32, device=self.device)
        self.ring_pos = torch.zeros(self.capacity, K, dtype=torch.int64, device=self.device)

    open_streams = property(lambda self: self.beats.open_streams)

    def samples_in(self, sid):
        return self.beats.samples_in(sid)

    def beats_in(self, sid):
        """beats the detector has given for this stream so far"""
        self.beats.samples_in(sid)
        return int(self.state.nb[sid])

    @torch.no_grad()
    def push(self, chunks, close=()):
        xs = as_chunks(chunks)
        sids, btab = self.state.plan({sid: tuple(x.shape) for sid, x in xs.items()}, tuple(close))      # (raises before anything changes)
        xp, x_total, _ = pack_chunks(xs, self.leads, self.device)
        return self.run(xp, x_total, sids, btab)

    def run(self, xp, x_total, sids, btab):
        """carry out a planned call: xp, x_total the chunks as `pack_chunks` packs them, sids and btab as planned ->
        {sid: (peaks, label, corr, rr_ratio)}; commits the plan"""
        dev, leads, lib = self.device, self.leads, _lib.lib()
        with torch.cuda.device(dev):
            new = self.beats.run(xp, x_total, sids, btab)      # the detector and the classifier read the same buffer
            tab = self.state.table(btab, [new[sid].numel() for sid in sids])
            new_total, out_total = int(tab["m"].sum()), int(tab["ne"].sum())
            new_pos = torch.cat([new[sid] for sid in sids]) if new_total else torch.zeros(1, dtype=torch.int64, device=dev)
            nbytes = scratch_bytes(lib.ral_rhythm_pool_scratch_bytes(new_total, leads, self.geom))
            scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
            out_pos = torch.empty(max(out_total, 1), dtype=torch.int64, device=dev)
            label = torch.empty(max(out_total, 1), dtype=torch.int32, device=dev)
            corr = torch.empty(max(out_total, 1), dtype=torch.float32, device=dev)
            rr = torch.empty(max(out_total, 1), dtype=torch.float32, device=dev)
            tab_dev = table_buffer(tab, dev)
            _lib.check(lib.ral_rhythm_pool(_ptr(self.beats.hist), _ptr(xp), x_total, tab.ctypes.data, len(tab), _ptr(tab_dev), 1,
                                           self.capacity, leads, self.geom, self.beats.hist_len, _ptr(self.ring),
                                           _ptr(self.ring_pos), _ptr(new_pos), new_total, _ptr(scratch), scratch.numel() * 4,
                                           _ptr(out_pos), _ptr(label), _ptr(corr), _ptr(rr), out_total, _stream()))
        self.state.commit(tab)
        return {sid: tuple(t[o:o + n] for t in (out_pos, label, corr, rr))
                for sid, o, n in zip(sids, tab["out_off"].tolist(), tab["ne"].tolist())}


class RhythmEvaluation:
    """What `evaluate_rhythm` returns: `clean`, `noisy`, `denoised`, the `BeatClasses` of the three records at the same beats
    `ref`; `mask` (R, cap) bool, the beats classified in all three; `truth` (m,) int64, 1 where the reference says V, for the
    beats of `mask` in record order; `scores` = {"noisy": {"acc", "precision", "f1"}, "denoised": {...}} from `scoring` (NaN
    where a ratio has no denominator)."""

    def __init__(self, clean, noisy, denoised, ref, mask, truth, scores):
        self.clean, self.noisy, self.denoised, self.ref = clean, noisy, denoised, ref
        self.mask, self.truth, self.scores = mask, truth, scores


def _score(logits, truth):
    out = {}
    for name, fn in (("acc", scoring.acc), ("precision", scoring.precision), ("f1", scoring.f1_score)):
        try:
            out[name] = fn(logits, truth)
        except ZeroDivisionError:
            out[name] = float("nan")
    return out


def evaluate_rhythm(denoiser, records, noise, snr_db, ref=None, ref_labels=None, offsets=None, rng=None, detector=None,
                    classifier=None):
    """The noise-stress protocol scored in beat classes, the reference's downstream question (test_cls.py) asked of a
    deterministic classifier: `mix_records(records, noise, snr_db, offsets, rng)`, `denoiser.denoise(noisy)`, then the clean, the
    noisy and the denoised records are classified AT THE SAME BEATS `ref` (`Beats` or per-record lists; default: the detections
    on the clean records), and `scoring.acc / precision / f1_score` of the noisy and of the denoised logits are taken against
    `ref_labels == 1` (per-record lists or an (R, cap) tensor of labels aligned with `ref`; default: the clean records' own
    labels), over the beats classified in all three -> `RhythmEvaluation`.  `denoiser` is a `StreamingDenoiser` or a
    `RateStreamingDenoiser`; detector and classifier (defaults `BeatDetector(fs)`, `BeatClassifier(fs)`) run at that object's
    outer rate `fs`."""
    fs, dev, clean, noisy, out = stress_front(denoiser, records, noise, snr_db, offsets, rng)
    cls = classifier or BeatClassifier(fs, device=dev)
    if ref is None:
        ref = (detector or BeatDetector(fs, device=dev)).detect(clean)
    c_clean = cls.classify(clean, ref)
    ref = Beats(c_clean.peaks, c_clean.count, fs)            # (lists are uploaded once)
    c_noisy, c_out = cls.classify(noisy, ref), cls.classify(out, ref)
    mask = c_clean.classified() & c_noisy.classified() & c_out.classified()
    if ref_labels is None:
        lab = c_clean.label
    elif torch.is_tensor(ref_labels):
        lab = ref_labels.to(mask.device)
    else:
        lab = torch.from_numpy(pad_rows(ref_labels, 0, np.int64, tuple(mask.shape))).to(mask.device)
    if lab.shape != mask.shape:
        raise _lib.RalError(f"evaluate_rhythm: ref_labels of shape {tuple(lab.shape)} for beats of shape {tuple(mask.shape)}")
    truth = (lab[mask] == 1).long()
    scores = {"noisy": _score(c_noisy.logits(mask)[0], truth), "denoised": _score(c_out.logits(mask)[0], truth)}
    return RhythmEvaluation(c_clean, c_noisy, c_out, ref, mask, truth, scores)
