"""The P-wave and ST-level measurement on the device: `PStMeasurer.measure` against the numpy oracle (tests/pst_util.py), the
interval conversions of `PStPoints` against the same formulas in numpy, `BeatTemplates.pst` against `measure` on the reshaped
templates, and `evaluate_pst` against its explicit composition.

The definition holds no contractible expression, so device and oracle are compared for exact equality of the three integers of
every beat and for bit equality of its ST levels, NaN positions included.  The conversions (fp64 formulas rounded to fp32) are
compared within 4 * 2^-24 relative."""
import functools

import numpy as np
import pytest
import torch

import beat_util as B
import pst_util as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 4 * 2.0 ** -24
KEYS = ("pon", "ppeak", "poff", "st", "on", "peaks", "count")


@functools.lru_cache(maxsize=None)
def _records(R, leads, T, seed, db=None):
    """-> (float32 (R, leads, T), truth lists, truth labels): synthetic rhythm records, clean or with `ma` noise at `db` dB"""
    from ecg_denoise_amd import synth
    x, beats, labels = synth.make_records_with_rhythm(R, leads, T, seed=seed, p_v=0.15)
    if db is not None:
        z = synth.make_noise_record("ma", leads, T, seed=seed + 100).astype(np.float64)
        x = B.add_noise(x.astype(np.float64), z, db).astype(np.float32)
    return x, beats, labels


def _dev(x):
    return x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _checked(pts, R, leads, fs):
    """the shape, type and padding checks of a `PStPoints` -> its tolist()"""
    cap = pts.peaks.shape[1]
    for t in (pts.pon, pts.ppeak, pts.poff):
        assert t.dtype == torch.int32 and t.is_cuda and tuple(t.shape) == (R, cap) and len(pts) == R
        for row, n in zip(t.tolist(), pts.count.tolist()):
            assert all(v == -1 for v in row[n:])
    assert pts.st.dtype == torch.float32 and pts.st.is_cuda and tuple(pts.st.shape) == (R, cap, leads)
    for r, n in enumerate(pts.count.tolist()):
        assert torch.isnan(pts.st[r, n:]).all()
    nan = torch.isnan(pts.st)
    assert torch.equal(nan.all(2), nan.any(2))                   # the ST level of every lead of a beat, or of none
    assert pts.fs == fs
    return pts.tolist()


def _measure(x, beats, fs=360, q0=0.15, **kw):
    """delineate, then measure -> (Fiducials, PStPoints, its tolist())"""
    from ecg_denoise_amd import BeatDelineator, PStMeasurer
    xd = _dev(x)
    f = BeatDelineator(fs, q0=q0, device=DEV).delineate(xd, beats)
    pts = PStMeasurer(fs, device=DEV, **kw).measure(xd, f)
    R, leads = (1, xd.shape[0]) if xd.dim() == 2 else xd.shape[:2]
    assert torch.equal(pts.on, f.on) and torch.equal(pts.peaks, f.peaks) and torch.equal(pts.count, f.count)
    return f, pts, _checked(pts, R, leads, fs)


def _against_oracle(x, f, got, fs=360, **kw):
    """every record against the oracle at the on and off the device was given, exactly -> the oracle's lists per record"""
    x = np.asarray(x.cpu() if torch.is_tensor(x) else x, dtype=np.float32)
    x = x[None] if x.ndim == 2 else x
    pos, count = f.peaks.tolist(), f.count.tolist()
    on, off = f.on.tolist(), f.off.tolist()
    return [P.compare(x[r], pos[r][:n], on[r][:n], off[r][:n], got[r], fs=fs, **kw) for r, n in enumerate(count)]


def _same(a, b):
    return all(torch.equal(torch.nan_to_num(getattr(a, k).double(), nan=-7.0), torch.nan_to_num(getattr(b, k).double(), nan=-7.0))
               and getattr(a, k).dtype == getattr(b, k).dtype for k in KEYS)


# ------------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("db", [None, 6.0])
def test_measure_equals_the_oracle_at_360_hz(db):
    """3 x 2 x 3 600, clean and with ma at 6 dB, at the generator's own beats"""
    x, truth, labels = _records(3, 2, 3600, 24, db)
    f, pts, got = _measure(x, truth)
    want = _against_oracle(x, f, got)
    assert sum(len(p) for p in truth) >= 30 and pts.count.tolist() == [len(p) for p in truth]
    if db is None:              # the clean records are measured: most beats have a P wave in front of the QRS, and an ST level
        found = [(a, b, c, o) for w, ons in zip(want, f.on.tolist()) for a, b, c, o in zip(w[0], w[1], w[2], ons) if b >= 0]
        assert len(found) >= 25 and all(0 <= a < b < c < o for a, b, c, o in found)
        assert sum(int(not np.isnan(s[0])) for w in want for s in w[3]) >= 30
    # another threshold is honoured
    f2, pts2, got2 = _measure(x, truth, p0=0.3)
    _against_oracle(x, f2, got2, p0=0.3)
    assert not torch.equal(pts2.ppeak, pts.ppeak) and _same_st(pts2, pts)


def _same_st(a, b):
    return P.same_bits(a.st.cpu().numpy(), b.st.cpu().numpy())


def test_measure_equals_the_oracle_at_500_hz_with_12_leads():
    """2 x 12 x 4 000: the same samples read at 500 Hz (Wp = 150: several rounds of the lane loops), p0 = 0.05"""
    x, truth, _ = _records(2, 12, 4000, 12)
    f, pts, got = _measure(x, truth, fs=500, q0=0.1, p0=0.05)
    want = _against_oracle(x, f, got, fs=500, p0=0.05)
    assert sum(len(p) for p in truth) >= 15 and any(v >= 0 for w in want for v in w[1])
    f1, pts1, got1 = _measure(torch.from_numpy(x[1]).to(DEV), [truth[1]], fs=500, q0=0.1, p0=0.05)      # a single record, (leads, T)
    assert got1[0][:3] == got[1][:3] and P.same_bits(np.array(got1[0][3], np.float32), np.array(got[1][3], np.float32))


# ------------------------------------------------------------------------------------------------ 2. edges
def test_records_with_0_1_and_2_beats_beats_at_both_ends_and_a_wider_cap():
    x, truth, _ = _records(3, 2, 3600, 24)
    T = x.shape[2]
    p = truth[0][3]
    for lists in ([[], [truth[1][2]], truth[2][4:6]], [[0, truth[0][2], T - 1], [0], [T - 1]], [[0, 1, 2], [T - 3, T - 2, T - 1], [p]]):
        f, pts, got = _measure(x, lists)
        assert pts.count.tolist() == [len(l) for l in lists] and pts.pon.shape[1] == max(1, max(len(l) for l in lists))
        _against_oracle(x, f, got)
    f, pts, got = _measure(x, [[], [truth[1][2]], truth[2][4:6]])
    assert got[0] == ([], [], [], []) and pts.pon[0].tolist() == [-1, -1] and torch.isnan(pts.st[0]).all()
    assert not np.isnan(got[1][3][0]).any() and not np.isnan(got[2][3][1]).any()
    # a Fiducials with a wider cap than any count, as the detector's Beats give: the padding is -1 / NaN, the beats are the same
    from ecg_denoise_amd import Beats
    pad = torch.full((3, 40), -1, dtype=torch.int32, device=DEV)
    pad[:, :2] = f.peaks
    f2, pts2, got2 = _measure(x, Beats(pad, f.count))
    assert tuple(pts2.pon.shape) == (3, 40) and tuple(pts2.st.shape) == (3, 40, 2)
    assert [g[:3] for g in got2] == [g[:3] for g in got]
    assert all(P.same_bits(np.array(a[3], np.float32).reshape(-1, 2), np.array(b[3], np.float32).reshape(-1, 2)) for a, b in zip(got, got2))


def test_two_beats_half_a_qrs_window_apart():
    """the first beat caps the second one's P search at 2/3 of their distance, behind its isoelectric sample: plo > phi, no P
    wave; the second caps the first one's ST sample away: NaN - and the same beat alone has both"""
    import delineate_util as U
    x, truth, _ = _records(3, 2, 3600, 24)
    p = truth[0][3]
    half = U.geometry(360)["Wq"] // 2
    lists = [[p, p + half], [p], [p - 400, p]]
    xx = x[:1].repeat(3, axis=0)
    f, pts, got = _measure(xx, lists)
    _against_oracle(xx, f, got)
    assert [g[1] for g in got[0][:3]] == [-1, -1, -1] and np.isnan(got[0][3][0]).all()
    assert got[1][1][0] > 0 and not np.isnan(got[1][3][0]).any()
    assert [g[0] for g in got[0][:3]] == [g[0] for g in got[1][:3]]           # the first beat's P wave does not depend on the next beat
    assert [g[1] for g in got[2][:3]] == [g[0] for g in got[1][:3]]           # a distant previous beat changes nothing


def test_short_and_constant_records():
    x, truth, _ = _records(3, 2, 3600, 24)
    p = truth[0][3]
    one = x[:1, :, p:p + 1]                                                    # T = 1
    f, pts, got = _measure(one, [[0]])
    assert got[0][:3] == ([-1], [-1], [-1]) and np.isnan(got[0][3]).all()
    _against_oracle(one, f, got)
    short = np.ascontiguousarray(x[:2, :, p - 15:p + 15])                      # T = 30 < Wp, around an R peak
    lists = [[15], [3, 15, 29]]
    f, pts, got = _measure(short, lists)
    _against_oracle(short, f, got)
    flat = np.full((2, 2, 900), 3.0, dtype=np.float32)                         # constant: the delineator finds no onset
    flat[1] = 1024.0
    lists = [[100, 300, 500, 700], [0, 450, 899]]
    f, pts, got = _measure(flat, lists)
    _against_oracle(flat, f, got)
    assert all(v == -1 for g in got for col in g[:3] for v in col) and torch.isnan(pts.st).all()
    assert torch.isnan(pts.pr_ms()).all() and torch.isnan(pts.p_ms()).all()
    # ... and with an onset and an offset put there by hand: s == 0 everywhere, no P wave, and an ST level of exactly 0
    from ecg_denoise_amd import PStMeasurer
    f.on, f.off = torch.clamp(f.peaks - 10, min=0), torch.clamp(f.peaks + 10, max=899)
    pts = PStMeasurer(device=DEV).measure(_dev(flat), f)
    got = _checked(pts, 2, 2, 360)
    _against_oracle(flat, f, got)
    assert (pts.ppeak == -1).all() and (pts.st[0] == 0).all() and (pts.st[1, :2] == 0).all()
    assert torch.isnan(pts.st[1, 2:]).all()                                    # 899 + 22 lies past the record; the padding


def test_on_and_off_that_do_not_bracket_the_beat_read_as_missing():
    """`on = p + 1`, `off = p - 1` and -1, all of them indices inside [-1, T - 1]: each reads as a missing point, as the oracle
    says - a missing on leaves nothing, a missing off leaves the P wave and takes the ST level"""
    from ecg_denoise_amd import Fiducials, PStMeasurer
    x, truth, _ = _records(3, 2, 3600, 24)
    T = x.shape[2]
    xd = _dev(x)
    f, pts, got = _measure(x, truth)
    live = torch.arange(f.peaks.shape[1], device=DEV)[None, :] < f.count[:, None]
    ms = PStMeasurer(device=DEV)
    for on, off in ((torch.clamp(f.peaks + 1, max=T - 1), f.off), (f.on, torch.clamp(f.peaks - 1, min=-1)),
                    (torch.full_like(f.on, -1), f.off), (f.on, torch.full_like(f.off, -1)),
                    (torch.clamp(f.peaks + 1, max=T - 1), torch.clamp(f.peaks - 1, min=-1))):
        assert int(on.min()) >= -1 and int(on.max()) <= T - 1 and int(off.min()) >= -1 and int(off.max()) <= T - 1
        g = Fiducials(on.contiguous(), off.contiguous(), f.tpeak, f.tend, f.peaks, f.count, f.fs)
        q = ms.measure(xd, g)
        _against_oracle(x, g, _checked(q, 3, 2, 360))
        if on is not f.on:
            assert (q.ppeak[live] == -1).all() and torch.isnan(q.st[live]).all()
        else:
            had = pts.ppeak >= 0                                  # (S over [on, p] is no larger: a P wave found stays found)
            assert int(had.sum()) >= 25 and all(torch.equal(getattr(q, k)[had], getattr(pts, k)[had]) for k in ("pon", "ppeak", "poff"))
            assert torch.isnan(q.st).all()


# ------------------------------------------------------------------------------------------------ 3. inputs
def test_beats_of_the_detector_and_the_same_positions_as_lists_give_identical_tensors():
    from ecg_denoise_amd import BeatDetector
    x, _, _ = _records(3, 2, 3600, 24, 6.0)
    xd = torch.from_numpy(x).to(DEV)
    det = BeatDetector(device=DEV).detect(xd)
    assert min(len(p) for p in det.tolist()) >= 5
    fa, a, _ = _measure(xd, det)
    fb, b, got = _measure(xd, det.tolist())
    n = b.pon.shape[1]
    assert n == max(det.count.tolist()) <= a.pon.shape[1]
    for k in ("pon", "ppeak", "poff", "on", "peaks"):
        assert torch.equal(getattr(a, k)[:, :n], getattr(b, k)) and (getattr(a, k)[:, n:] == -1).all(), k
    assert P.same_bits(a.st[:, :n].cpu().numpy(), b.st.cpu().numpy()) and torch.isnan(a.st[:, n:]).all()
    assert torch.equal(a.count, b.count)
    _against_oracle(x, fb, got)


def test_a_non_contiguous_fp64_input_equals_its_contiguous_fp32_copy():
    x, truth, _ = _records(3, 2, 3600, 24, 6.0)
    wide = torch.from_numpy(x).to(DEV).double().permute(0, 2, 1).contiguous().permute(0, 2, 1)      # (R, leads, T) over (R, T, leads)
    assert not wide.is_contiguous() and wide.dtype == torch.float64
    _, a, _ = _measure(wide, truth)
    _, b, _ = _measure(x, truth)
    assert _same(a, b) and _same_st(a, b)


def test_refusals_on_the_device():
    from ecg_denoise_amd import BeatDelineator, Fiducials, PStMeasurer, RalError
    ms = PStMeasurer(device=DEV)
    x = torch.zeros(2, 2, 1000, device=DEV)
    z = lambda *s: torch.zeros(*s, dtype=torch.int32, device=DEV)
    with pytest.raises(RalError, match="PStMeasurer.measure: 1 beat lists on cuda:0 for 2 records on cuda:0"):
        ms.measure(x, Fiducials(z(1, 4), z(1, 4), z(1, 4), z(1, 4), z(1, 4), z(1)))
    with pytest.raises(RalError, match="PStMeasurer.measure: 2 beat lists on cpu for 2 records on cuda:0"):
        ms.measure(x, Fiducials(*(torch.zeros(2, 4, dtype=torch.int32) for _ in range(5)), torch.zeros(2, dtype=torch.int32)))
    R = 65536
    with pytest.raises(RalError, match="pst_records: need 1 <= R <= 65535"):
        ms.measure(torch.zeros(R, 1, 8, device=DEV), Fiducials(z(R, 1), z(R, 1), z(R, 1), z(R, 1), z(R, 1), z(R)))
    f = BeatDelineator(device=DEV).delineate(x, [[100, 500], [300]])          # ... and what the delineator gives is taken
    assert tuple(ms.measure(x, f).st.shape) == (2, 2, 2)


# ------------------------------------------------------------------------------------------------ 4. intervals
def test_intervals_are_the_formulas_on_the_device_integers():
    x, truth, _ = _records(3, 2, 3600, 24)
    for fs, q0 in ((360, 0.15), (500, 0.1)):
        f, pts, got = _measure(x, truth, fs=fs, q0=q0)
        pon, poff, on = (t.cpu().numpy().astype(np.float64) for t in (pts.pon, pts.poff, pts.on))
        pr = np.where((pon >= 0) & (on >= 0), (on - pon) * 1000.0 / fs, np.nan)
        pd = np.where((pon >= 0) & (poff >= 0), (poff - pon) * 1000.0 / fs, np.nan)
        for name, want in (("pr_ms", pr), ("p_ms", pd)):
            mine = getattr(pts, name)()
            assert mine.dtype == torch.float32 and mine.is_cuda and mine.shape == pts.pon.shape, name
            mine = mine.cpu().numpy().astype(np.float64)
            assert np.array_equal(np.isnan(mine), np.isnan(want)), name
            ok = ~np.isnan(want)
            assert ok.sum() >= 15 and np.all(np.abs(mine[ok] - want[ok]) <= RTOL * np.abs(want[ok])), (name, fs)
        m = pts.measurable()
        assert set(m) == {"p", "st"}
        assert np.array_equal(np.isnan(pr), ~m["p"].cpu().numpy())
        assert np.array_equal(np.isnan(pts.st.cpu().numpy()).all(2), ~m["st"].cpu().numpy())
    assert 100.0 < np.nanmedian(pr) * 500 / 360 < 280.0                       # (read at 360 Hz: a PR interval)


# ------------------------------------------------------------------------------------------------ 5. templates
def test_templates_pst_is_measure_on_the_reshaped_templates():
    """2 x 2 x 7 200: two windows of 10 s per record; a template's beat has no neighbour"""
    from ecg_denoise_amd import Beats, BeatDelineator, MedianBeat, PStMeasurer
    x, truth, labels = _records(2, 2, 7200, 24)
    xd = _dev(x)
    tpl = MedianBeat(device=DEV).average(xd, truth, labels)
    R, nw, leads, Wn = tpl.template.shape
    assert (R, nw, leads) == (2, 2, 2) and int(tpl.used.min()) >= 3
    mine = tpl.pst()
    flat = tpl.template.view(R * nw, leads, Wn)
    one = Beats(torch.full((R * nw, 1), tpl.center, dtype=torch.int32, device=DEV), torch.ones(R * nw, dtype=torch.int32, device=DEV))
    f = BeatDelineator(device=DEV).delineate(flat, one)
    want = PStMeasurer(device=DEV).measure(flat, f)
    assert _same(mine, want) and _same_st(mine, want)
    got = _checked(mine, R * nw, leads, 360)
    _against_oracle(flat, f, got)
    assert (mine.ppeak >= 0).all() and not torch.isnan(mine.st).any()         # a clean median N beat has a P wave and an ST level
    assert ((mine.pon < mine.ppeak) & (mine.ppeak < mine.poff) & (mine.poff < mine.on)).all()
    # min_beats above what a window has: no beat, the padding everywhere; another threshold reaches the measurer
    none = tpl.pst(min_beats=10 ** 6)
    assert none.count.tolist() == [0] * (R * nw) and (none.ppeak == -1).all() and torch.isnan(none.st).all()
    high = tpl.pst(measurer=PStMeasurer(p0=10.0, device=DEV))
    assert (high.ppeak == -1).all() and _same_st(high, mine)


# ------------------------------------------------------------------------------------------------ 6. composition
def _nan_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.isnan(a), torch.isnan(b)) and \
        torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0))


def _scores_explicit(pc, po):
    """the score formulas, written out -> (p share (R,), PR MAE (R,), ST MAE (R, leads), pooled dict)"""
    pc_p, po_p = pc.ppeak >= 0, po.ppeak >= 0
    both = pc_p & po_p
    err = (po.pr_ms().double() - pc.pr_ms().double()).abs()
    err = torch.where(both, err, torch.zeros_like(err))
    share, pr = both.sum(1).double() / pc_p.sum(1).double(), err.sum(1) / both.sum(1).double()
    nb, nc = int(both.sum()), int(pc_p.sum())
    pooled = {"p_share": nb / nc if nc else float("nan"), "pr_mae_ms": float(err.sum()) / nb if nb else float("nan"), "p_beats": nb}
    sb = ~torch.isnan(pc.st[..., 0]) & ~torch.isnan(po.st[..., 0])
    serr = (po.st.double() - pc.st.double()).abs()
    serr = torch.where(sb[..., None], serr, torch.zeros_like(serr))
    st = serr.sum(1) / sb.sum(1).double()[:, None]
    ns = int(sb.sum())
    pooled["st_mae"] = (serr.sum((0, 1)) / ns).tolist() if ns else [float("nan")] * pc.st.shape[2]
    pooled["st_beats"] = ns
    return share, pr, st, pooled


def _pooled_equal(a, b):
    flat = lambda d: [v for k in sorted(d) for v in (d[k] if isinstance(d[k], list) else [d[k]])]
    return sorted(a) == sorted(b) and all(x == y or (np.isnan(x) and np.isnan(y)) for x, y in zip(flat(a), flat(b)))


@pytest.mark.parametrize("fs", [360, 500])
def test_evaluate_pst_is_the_explicit_composition(fs):
    """with a freshly initialised model: the plumbing, not an improvement (an untrained model promises none)"""
    from ecg_denoise_amd import (BeatDelineator, BeatDetector, ClassicalDenoiser, PStMeasurer, RateStreamingDenoiser, UNet, evaluate_pst,
                                 mix_records, pst_scores, synth)
    from ecg_denoise_amd.infer import StreamingDenoiser
    model = UNet(leads=2, L=64, max_batch=16, train=False, device=DEV, seed=11).eval()
    T = 3600
    x, truth, _ = _records(3, 2, T, 24)
    rec = torch.from_numpy(x).to(DEV)
    noise = torch.from_numpy(synth.make_noise_record("ma", 2, T + 500, seed=3)).to(DEV)
    dn = StreamingDenoiser(model, use_graph=False) if fs == 360 else RateStreamingDenoiser(model, fs, use_graph=False)
    offs = [5, 200, 499]
    ev = evaluate_pst(dn, rec, noise, 6.0, offsets=offs)
    noisy, clean = mix_records(rec, noise, 6.0, offsets=offs)
    ref = BeatDetector(fs, device=DEV).detect(clean)
    dl, ms = BeatDelineator(fs, device=DEV), PStMeasurer(fs, device=DEV)
    pc, pn, pd = (ms.measure(y, dl.delineate(y, ref)) for y in (clean, noisy, dn.denoise(noisy)))
    assert ev.ref.tolist() == ref.tolist() and min(len(p) for p in ref.tolist()) >= 4
    assert all(_same(a, b) and _same_st(a, b) for a, b in ((ev.clean, pc), (ev.noisy, pn), (ev.denoised, pd)))
    assert torch.equal(ev.fiducials["noisy"].off, dl.delineate(noisy, ref).off) and set(ev.fiducials) == {"clean", "noisy", "denoised"}
    assert int((pc.ppeak >= 0).sum()) >= 6 and int((~torch.isnan(pc.st[..., 0])).sum()) >= 6
    for key, po in (("noisy", pn), ("denoised", pd)):
        share, pr, st, pooled = _scores_explicit(pc, po)
        assert set(ev.share[key]) == {"p"} and set(ev.mae[key]) == {"pr_ms", "st"}
        assert _nan_equal(ev.share[key]["p"], share) and _nan_equal(ev.mae[key]["pr_ms"], pr)
        assert tuple(ev.mae[key]["st"].shape) == (3, 2) and _nan_equal(ev.mae[key]["st"], st)
        assert _pooled_equal(ev.pooled[key], pooled)
        assert _pooled_equal(pst_scores(pc, po, rows=torch.tensor([0, 2], device=DEV))[2],
                             _scores_explicit(*(_rows(q, [0, 2]) for q in (pc, po)))[3])
    if fs == 360:               # a reference given by the caller, per-record SNRs, and a classical denoiser in place of the model
        fft = ClassicalDenoiser("fft", 1000, device=DEV)
        ev2 = evaluate_pst(fft, rec, noise, [0.0, 6.0, 12.0], ref=truth, offsets=offs)
        assert ev2.ref.tolist() == truth and set(ev2.pooled) == {"noisy", "denoised"}
        n2, c2 = mix_records(rec, noise, [0.0, 6.0, 12.0], offsets=offs)
        want = ms.measure(c2, dl.delineate(c2, truth))
        assert _same(ev2.clean, want) and _same_st(ev2.clean, want)
        o2 = fft.denoise(n2)
        want = ms.measure(o2, dl.delineate(o2, truth))
        assert _same(ev2.denoised, want) and _same_st(ev2.denoised, want)
        assert _pooled_equal(ev2.pooled["denoised"], _scores_explicit(ev2.clean, want)[3])


def _rows(p, idx):
    from ecg_denoise_amd import PStPoints
    return PStPoints(*(getattr(p, k)[idx] for k in KEYS), p.fs)
