"""The median beat on the device: `MedianBeat.average` against the numpy oracle (tests/template_util.py), `BeatTemplates
.delineate` against the delineator's oracle on the oracle's templates, `.intervals` against the same formulas in numpy, and
`evaluate_templates` against its explicit composition.

The definition holds no contractible expression, so device and oracle are compared for exact equality of values.  The interval
conversions (fp64 formulas rounded to fp32) are compared within 4 * 2^-24 relative."""
import functools

import numpy as np
import pytest
import torch

import delineate_util as D
import template_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 4 * 2.0 ** -24
KEYS = ("template", "used", "total", "rr")


@functools.lru_cache(maxsize=None)
def _records(R, leads, T, seed):
    """-> (float32 (R, leads, T), truth lists, truth labels): the synthetic rhythm records of the delineator's tests"""
    from ecg_denoise_amd import synth
    return synth.make_records_with_rhythm(R, leads, T, seed=seed, p_v=0.15)


def _average(x, beats, classes=None, fs=360, **kw):
    """-> BeatTemplates after the shape, type and geometry checks"""
    from ecg_denoise_amd import MedianBeat
    xd = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    t = MedianBeat(fs, device=DEV, **kw).average(xd, beats, classes)
    R, leads, T = (1,) + tuple(xd.shape) if xd.dim() == 2 else tuple(xd.shape)
    g = U.geometry(fs, kw.get("win_s", 10), kw.get("hop_s", 10))
    nw = len(U.windows(T, g))
    assert t.template.dtype == torch.float32 and t.template.is_cuda and tuple(t.template.shape) == (R, nw, leads, g["Wn"])
    for v in (t.used, t.total, t.rr):
        assert v.dtype == torch.int32 and v.is_cuda and tuple(v.shape) == (R, nw)
    assert t.index.dtype == np.int64 and t.index.tolist() == [list(w) for w in U.windows(T, g)]
    assert len(t) == R and t.center == g["Wpre"] and t.fs == fs and t.geometry == g
    return t


def _oracle(x, lists, labels, fs=360, win_s=10, hop_s=10):
    return U.median_beats_records(np.asarray(x, dtype=np.float32), lists, labels, U.geometry(fs, win_s, hop_s))


def _same(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in KEYS)


# ------------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("with_labels", [True, False])
def test_templates_equal_the_oracle_at_360_hz(with_labels):
    """3 x 2 x 3 600, win_s = 4, hop_s = 2: four windows of 1 440 samples, every beat in two of them"""
    x, truth, labels = _records(3, 2, 3600, 24)
    lab = labels if with_labels else None
    t = _average(x, truth, lab, win_s=4, hop_s=2)
    want = _oracle(x, truth, lab, win_s=4, hop_s=2)
    U.compare(t, want)
    assert want["used"].shape == (3, 4) and want["used"].min() >= 2 and want["rr"].min() > 100
    if with_labels:          # the V beats are left out: fewer members than without labels, in some window
        assert (want["total"] < _oracle(x, truth, None, win_s=4, hop_s=2)["total"]).any()


def test_templates_equal_the_oracle_at_500_hz_with_12_leads():
    """2 x 12 x 4 000 read at 500 Hz, win_s = 8: one window; Wn = 501: 16 tiles, the last of 21 samples"""
    x, truth, labels = _records(2, 12, 4000, 12)
    t = _average(x, truth, labels, fs=500, win_s=8)
    want = _oracle(x, truth, labels, fs=500, win_s=8)
    U.compare(t, want)
    assert want["used"].shape == (2, 1) and want["used"].min() >= 5
    one = _average(torch.from_numpy(x[1]).to(DEV), [truth[1]], [labels[1]], fs=500, win_s=8)          # a single record, (leads, T)
    assert all(torch.equal(getattr(one, k)[0], getattr(t, k)[1]) for k in KEYS)


# ------------------------------------------------------------------------------------------------ 2. counts and ties
@functools.lru_cache(maxsize=None)
def _tied():
    """8 records of 1 x 6 000 quantised to quarters (ties are certain), some samples -0.0; beats 200 + 20 j; list lengths around
    the wave (64) and KMAX (256) boundaries"""
    rng = np.random.default_rng(7)
    x = (np.round(4 * rng.standard_normal((8, 1, 6000))) / 4).astype(np.float32)
    x[:, :, ::5][x[:, :, ::5] == 0] = np.float32(-0.0)
    assert np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    lists = [[200 + 20 * j for j in range(n)] for n in (1, 2, 63, 64, 65, 255, 256, 257)]
    return x, lists


def test_counts_around_the_wave_and_kmax_boundaries_with_tied_samples():
    x, lists = _tied()
    T = x.shape[2]
    t = _average(x, lists, win_s=U.Fraction(T, 360))            # W = T: one window
    want = _oracle(x, lists, None, win_s=U.Fraction(T, 360))
    U.compare(t, want)
    assert want["used"][:, 0].tolist() == [1, 2, 63, 64, 65, 255, 256, 256] and want["total"][:, 0].tolist()[-1] == 257
    assert want["rr"][:, 0].tolist() == [-1] + [20] * 7
    # heavily overlapping members: 5 s windows every second
    t = _average(x, lists, win_s=5, hop_s=1)
    want = _oracle(x, lists, None, win_s=5, hop_s=1)
    U.compare(t, want)
    assert want["used"].shape == (8, 12) and want["used"].max() == 90 and (want["used"] == 0).any()


def test_lead_groups_of_every_size():
    """5 leads with 100, 60, 40 and 7 beats: the kernel stages 2, 4, 5 and 5 leads together (as many as 256 // used, at most
    16), so the last group of the first two records is a partial one"""
    rng = np.random.default_rng(11)
    x = (np.round(8 * rng.standard_normal((4, 5, 3000))) / 8).astype(np.float32)
    lists = [[200 + 9 * j for j in range(n)] for n in (100, 60, 40, 7)]
    t = _average(x, lists)
    want = _oracle(x, lists, None)
    U.compare(t, want)
    assert want["used"][:, 0].tolist() == [100, 60, 40, 7]


# ------------------------------------------------------------------------------------------------ 3. edges
def test_empty_lists_boundary_beats_excluded_labels_a_wider_cap_and_short_records():
    from ecg_denoise_amd import Beats
    x, truth, labels = _records(3, 2, 3600, 24)
    T, g = x.shape[2], U.geometry(360)
    pre, post = g["Wpre"], g["Wpost"]
    # empty lists, and beats at both ends of the membership rule
    edge = [0, pre - 1, pre, T - 1 - post, T - post, T - 1]
    lists = [[], edge, truth[2]]
    t = _average(x, lists)
    want = _oracle(x, lists, None)
    U.compare(t, want)
    assert want["used"][:, 0].tolist()[:2] == [0, 2] and want["rr"][:2, 0].tolist() == [-1, 1]
    assert not t.template[0].any() and t.template[1].any()
    # every label V or -1: zeros, used = 0, rr = -1
    bad = [[1] * len(truth[0]), [-1] * len(truth[1]), [1, -1] * (len(truth[2]) // 2) + [1] * (len(truth[2]) % 2)]
    t = _average(x, truth, bad)
    U.compare(t, _oracle(x, truth, bad))
    assert not t.template.any() and not t.used.any() and not t.total.any() and (t.rr == -1).all()
    # a Beats (and BeatClasses-shaped labels on the device) with a cap wider than any count
    a = _average(x, truth, labels)
    cap = max(len(p) for p in truth) + 9
    peaks = torch.full((3, cap), -1, dtype=torch.int32, device=DEV)
    lab = torch.full((3, cap), -1, dtype=torch.int32, device=DEV)
    for r in range(3):
        peaks[r, :len(truth[r])] = torch.tensor(truth[r], dtype=torch.int32)
        lab[r, :len(truth[r])] = torch.tensor(labels[r], dtype=torch.int32)
    count = torch.tensor([len(p) for p in truth], dtype=torch.int32, device=DEV)
    b = _average(x, Beats(peaks, count), lab)
    assert _same(a, b)
    U.compare(b, _oracle(x, truth, labels))
    # T < Wn: no beat fits; T < W: the single window [0, T)
    short = np.ascontiguousarray(x[:, :, :g["Wn"] - 1])
    t = _average(short, [[pre], [5, 100], []])
    U.compare(t, _oracle(short, [[pre], [5, 100], []], None))
    assert not t.used.any() and t.index.tolist() == [[0, g["Wn"] - 1]]
    part = np.ascontiguousarray(x[:, :, :2000])
    cut = [[p for p in row if p < 2000] for row in truth]
    t = _average(part, cut)
    U.compare(t, _oracle(part, cut, None))
    assert t.index.tolist() == [[0, 2000]] and int(t.used.min()) >= 2


# ------------------------------------------------------------------------------------------------ 4. delineation and intervals
def test_delineate_and_intervals_of_the_templates():
    x, truth, labels = _records(3, 2, 3600, 24)
    fs, g = 360, U.geometry(360, 4, 2)
    t = _average(x, truth, labels, win_s=4, hop_s=2)
    want = _oracle(x, truth, labels, win_s=4, hop_s=2)
    U.compare(t, want)
    R, nw = want["used"].shape
    lo = int(np.sort(want["used"].reshape(-1))[R * nw // 2])              # a min_beats that some windows miss and some meet
    assert want["used"].min() < lo <= want["used"].max()
    for mb in (3, lo):
        f = t.delineate(min_beats=mb)
        for k in ("on", "off", "tpeak", "tend"):
            v = getattr(f, k)
            assert v.dtype == torch.int32 and tuple(v.shape) == (R * nw, 1)
        got = np.stack([getattr(f, k).cpu().numpy()[:, 0] for k in ("on", "off", "tpeak", "tend")], axis=1).reshape(R, nw, 4)
        assert f.count.tolist() == (want["used"].reshape(-1) >= mb).astype(int).tolist()
        theirs = np.array([[D.delineate_beat(want["template"][r, w], g["Wpre"], None, fs) if want["used"][r, w] >= mb else (-1,) * 4
                            for w in range(nw)] for r in range(R)])
        assert np.array_equal(got, theirs)
        on, off, tend = (theirs[..., k].astype(np.float64) for k in (0, 1, 3))
        rr = want["rr"].astype(np.float64)
        qrs = np.where((on >= 0) & (off >= 0), (off - on) * 1000.0 / fs, np.nan)
        qt = np.where((on >= 0) & (tend >= 0), (tend - on) * 1000.0 / fs, np.nan)
        with np.errstate(invalid="ignore"):
            qtc = qt / np.sqrt(np.where(rr >= 0, rr / fs, np.nan))
        iv = t.intervals(min_beats=mb)
        assert set(iv) == {"qrs_ms", "qt_ms", "qtc_ms"}
        for name, ref in (("qrs_ms", qrs), ("qt_ms", qt), ("qtc_ms", qtc)):
            mine = iv[name]
            assert mine.dtype == torch.float32 and mine.is_cuda and tuple(mine.shape) == (R, nw), name
            mine = mine.cpu().numpy().astype(np.float64)
            assert np.array_equal(np.isnan(mine), np.isnan(ref)), name
            ok = ~np.isnan(ref)
            assert ok.sum() >= 3 and np.all(np.abs(mine[ok] - ref[ok]) <= RTOL * np.abs(ref[ok])), name
    assert np.isnan(qrs).any() and 60.0 < np.nanmedian(qrs) < 140.0 and 250.0 < np.nanmedian(qtc) < 550.0
    # rr < 0 leaves QTc alone undetermined: a record whose one used beat is the first of its list
    p = truth[0][3]
    one = _average(x[:1], [[p]])
    iv = one.intervals(min_beats=1)
    assert int(one.rr) == -1 and not torch.isnan(iv["qt_ms"]).any() and torch.isnan(iv["qtc_ms"]).all()


# ------------------------------------------------------------------------------------------------ 5. determinism
def test_two_calls_agree_and_a_record_alone_equals_its_row_in_a_batch():
    x, truth, labels = _records(3, 2, 3600, 24)
    a = _average(x, truth, labels, win_s=4, hop_s=2)
    b = _average(x, truth, labels, win_s=4, hop_s=2)
    assert _same(a, b)
    for r in range(3):
        one = _average(x[r:r + 1], [truth[r]], [labels[r]], win_s=4, hop_s=2)
        assert all(torch.equal(getattr(one, k)[0], getattr(a, k)[r]) for k in KEYS), r
    xt, lists = _tied()
    c = _average(xt, lists, win_s=5, hop_s=1)
    one = _average(xt[7:], lists[7:], win_s=5, hop_s=1)
    assert all(torch.equal(getattr(one, k)[0], getattr(c, k)[7]) for k in KEYS)


# ------------------------------------------------------------------------------------------------ 6. composition
def _nan_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.isnan(a), torch.isnan(b)) and \
        torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0))


@pytest.mark.parametrize("fs", [360, 500])
def test_evaluate_templates_is_the_explicit_composition(fs):
    """with a freshly initialised model: the plumbing, not an improvement (an untrained model promises none)"""
    from ecg_denoise_amd import (BeatClassifier, BeatDelineator, BeatDetector, ClassicalDenoiser, MedianBeat, RateStreamingDenoiser,
                                 UNet, evaluate_templates, interval_scores, mix_records, synth)
    from ecg_denoise_amd.infer import StreamingDenoiser
    model = UNet(leads=2, L=64, max_batch=16, train=False, device=DEV, seed=11).eval()
    T = 3600
    x, truth, labels = _records(3, 2, T, 24)
    rec = torch.from_numpy(x).to(DEV)
    noise = torch.from_numpy(synth.make_noise_record("ma", 2, T + 500, seed=3)).to(DEV)
    dn = StreamingDenoiser(model, use_graph=False) if fs == 360 else RateStreamingDenoiser(model, fs, use_graph=False)
    offs = [5, 200, 499]
    avg = MedianBeat(fs, win_s=4, hop_s=2, device=DEV)
    ev = evaluate_templates(dn, rec, noise, 6.0, offsets=offs, averager=avg)
    noisy, clean = mix_records(rec, noise, 6.0, offsets=offs)
    ref = BeatDetector(fs, device=DEV).detect(clean)
    cls = BeatClassifier(fs, device=DEV).classify(clean, ref)
    dl = BeatDelineator(fs, device=DEV)
    tc, tn, td = avg.average(clean, ref, cls), avg.average(noisy, ref, cls), avg.average(dn.denoise(noisy), ref, cls)
    assert ev.ref.tolist() == ref.tolist() and torch.equal(ev.labels, cls.label) and min(len(p) for p in ref.tolist()) >= 4
    assert _same(ev.clean, tc) and _same(ev.noisy, tn) and _same(ev.denoised, td)
    ok = tc.used >= 3
    assert ev.windows == int(ok.sum()) >= 3
    fc = tc.delineate(dl)
    for key, t in (("noisy", tn), ("denoised", td)):
        se = (t.template.double() - tc.template.double()).pow(2).sum((2, 3))
        per = 2 * tc.template.shape[3]
        assert _nan_equal(ev.rmse[key], torch.where(ok, torch.sqrt(se / per), torch.full_like(se, float("nan"))))
        assert ev.pooled_rmse[key] == float(torch.sqrt(se[ok].sum() / (int(ok.sum()) * per)))
        f = t.delineate(dl)
        for k in ("on", "off", "tpeak", "tend", "count"):
            assert torch.equal(getattr(ev.fiducials[key], k), getattr(f, k)), (key, k)
        share, mae, pooled = interval_scores(fc, f)
        assert ev.pooled[key] == pooled or all(v == pooled[k] or (np.isnan(v) and np.isnan(pooled[k])) for k, v in ev.pooled[key].items())
        for name in ("qrs", "qt"):
            assert _nan_equal(ev.share[key][name], share[name].view(ok.shape)) and _nan_equal(ev.mae_ms[key][name], mae[name].view(ok.shape))
    assert ev.pooled_rmse["noisy"] > 0
    if fs == 360:               # beats and labels given by the caller, per-record SNRs, a classical denoiser, min_beats
        cd = ClassicalDenoiser("fft", 1000, device=DEV)
        ev2 = evaluate_templates(cd, rec, noise, [0.0, 6.0, 12.0], ref=truth, ref_labels=labels, offsets=offs, averager=avg, min_beats=4)
        n2, c2 = mix_records(rec, noise, [0.0, 6.0, 12.0], offsets=offs)
        assert ev2.ref.tolist() == truth and _same(ev2.clean, avg.average(c2, truth, labels))
        assert _same(ev2.denoised, avg.average(cd.denoise(n2), truth, labels))
        assert ev2.windows == int((ev2.clean.used >= 4).sum()) and torch.equal(torch.isnan(ev2.rmse["noisy"]), ev2.clean.used < 4)
        assert ev2.fiducials["clean"].count.tolist() == (ev2.clean.used.reshape(-1) >= 4).int().tolist()
