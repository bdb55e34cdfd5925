"""Beat delineation on the device: `BeatDelineator.delineate` against the numpy oracle (tests/delineate_util.py), the interval
conversions of `Fiducials` against the same formulas in numpy, and `evaluate_intervals` against its explicit composition.

The definition holds no contractible expression, so device and oracle are compared for exact equality of all four integers of
every beat.  The conversions (fp64 formulas rounded to fp32) are compared within 4 * 2^-24 relative."""
import functools

import numpy as np
import pytest
import torch

import beat_util as B
import delineate_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 4 * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _records(R, leads, T, seed, db=None):
    """-> (float32 (R, leads, T), truth lists, truth labels): synthetic rhythm records, clean or with `ma` noise at `db` dB"""
    from ecg_denoise_amd import synth
    x, beats, labels = synth.make_records_with_rhythm(R, leads, T, seed=seed, p_v=0.15)
    if db is not None:
        z = synth.make_noise_record("ma", leads, T, seed=seed + 100).astype(np.float64)
        x = B.add_noise(x.astype(np.float64), z, db).astype(np.float32)
    return x, beats, labels


def _delineate(x, beats, fs=360, **kw):
    """-> (Fiducials, its tolist()) after the shape, type and padding checks"""
    from ecg_denoise_amd import BeatDelineator
    xd = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    f = BeatDelineator(fs, device=DEV, **kw).delineate(xd, beats)
    R = 1 if xd.dim() == 2 else xd.shape[0]
    for t in (f.on, f.off, f.tpeak, f.tend):
        assert t.dtype == torch.int32 and t.is_cuda and t.shape == f.peaks.shape and t.shape[0] == R == len(f)
        for row, n in zip(t.tolist(), f.count.tolist()):
            assert all(v == -1 for v in row[n:])
    assert f.fs == fs
    return f, f.tolist()


def _against_oracle(x, lists, got, fs=360, **kw):
    """every record against the oracle, exactly -> the oracle's lists per record"""
    return [U.compare(np.asarray(x[r], dtype=np.float32), lists[r], got[r], fs=fs, **kw) for r in range(len(lists))]


def _same(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("on", "off", "tpeak", "tend", "peaks", "count"))


# ------------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("db", [None, 6.0])
def test_delineate_equals_the_oracle_at_360_hz(db):
    """3 x 2 x 3 600, clean and with ma at 6 dB, at the generator's own beats"""
    x, truth, labels = _records(3, 2, 3600, 24, db)
    f, got = _delineate(x, truth)
    want = _against_oracle(x, truth, got)
    assert sum(len(p) for p in truth) >= 30 and f.count.tolist() == [len(p) for p in truth]
    if db is None:              # the clean records are delineated: most beats have all four points, in their order
        whole = [(a, b, c, d) for w in want for a, b, c, d in zip(*w) if d >= 0]
        assert len(whole) >= 25 and all(0 <= a < b < c < d for a, b, c, d in whole)
    # another threshold is honoured
    f2, got2 = _delineate(x, truth, q0=0.3)
    _against_oracle(x, truth, got2, q0=0.3)
    assert not torch.equal(f2.on, f.on)


def test_delineate_equals_the_oracle_at_500_hz_with_12_leads():
    """2 x 12 x 4 000: the same samples read at 500 Hz (Wq = 60, Wt = 275: several rounds of the lane loops), q0 = 0.1"""
    x, truth, _ = _records(2, 12, 4000, 12)
    f, got = _delineate(x, truth, fs=500, q0=0.1)
    want = _against_oracle(x, truth, got, fs=500, q0=0.1)
    assert sum(len(p) for p in truth) >= 15 and any(v >= 0 for w in want for v in w[3])
    f1, got1 = _delineate(torch.from_numpy(x[1]).to(DEV), [truth[1]], fs=500, q0=0.1)      # a single record, (leads, T)
    assert got1[0] == got[1]


# ------------------------------------------------------------------------------------------------ 2. edges
def test_records_with_0_1_and_2_beats_beats_at_both_ends_and_a_wider_cap():
    x, truth, _ = _records(3, 2, 3600, 24)
    T = x.shape[2]
    p = truth[0][3]
    for lists in ([[], [truth[1][2]], truth[2][4:6]], [[0, truth[0][2], T - 1], [0], [T - 1]], [[0, 1, 2], [T - 3, T - 2, T - 1], [p]]):
        f, got = _delineate(x, lists)
        assert f.count.tolist() == [len(l) for l in lists] and f.on.shape[1] == max(1, max(len(l) for l in lists))
        _against_oracle(x, lists, got)
    f, got = _delineate(x, [[], [truth[1][2]], truth[2][4:6]])
    assert got[0] == ([], [], [], []) and 0 <= got[1][0][0] < truth[1][2] < got[1][1][0] and f.on[0].tolist() == [-1, -1]
    # a Beats with a wider cap than any count, as the detector gives: the padding is -1 and the beats are the same
    from ecg_denoise_amd import Beats
    pad = torch.full((3, 40), -1, dtype=torch.int32, device=DEV)
    pad[:, :2] = f.peaks
    f2, got2 = _delineate(x, Beats(pad, f.count))
    assert tuple(f2.on.shape) == (3, 40) and got2 == got


def test_two_beats_half_a_qrs_window_apart():
    """the second beat caps the first one's T search at 2/3 of their distance: lim = p + 14 < off + gt, no T wave - and the
    same beat alone has one"""
    x, truth, _ = _records(3, 2, 3600, 24)
    p = truth[0][3]
    half = U.geometry(360)["Wq"] // 2
    lists = [[p, p + half], [p], [p, p + 3 * U.geometry(360)["Wt"] // 2]]
    f, got = _delineate(x[:1].repeat(3, axis=0), lists)
    _against_oracle(x[:1].repeat(3, axis=0), lists, got)
    assert got[0][2][0] == got[0][3][0] == -1 and got[1][3][0] > got[1][2][0] > p
    assert [g[0] for g in got[0][:2]] == [g[0] for g in got[1][:2]]           # the QRS bounds do not depend on the next beat
    assert [g[0] for g in got[2]] == [g[0] for g in got[1]]                   # a distant next beat changes nothing


def test_short_and_constant_records():
    x, truth, _ = _records(3, 2, 3600, 24)
    p = truth[0][3]
    one = x[:1, :, p:p + 1]                                                    # T = 1
    f, got = _delineate(one, [[0]])
    assert got[0] == ([-1], [-1], [-1], [-1])
    _against_oracle(one, [[0]], got)
    short = np.ascontiguousarray(x[:2, :, p - 15:p + 15])                      # T = 30 < Wq, around an R peak
    lists = [[15], [3, 15, 29]]
    f, got = _delineate(short, lists)
    _against_oracle(short, lists, got)
    assert all(v == -1 for g in got for v in g[2] + g[3])
    flat = np.full((2, 2, 900), 3.0, dtype=np.float32)                         # constant: A == 0, every point is -1
    flat[1] = 1024.0
    lists = [[100, 300, 500, 700], [0, 450, 899]]
    f, got = _delineate(flat, lists)
    _against_oracle(flat, lists, got)
    assert all(v == -1 for g in got for col in g for v in col)
    assert torch.isnan(f.qrs_ms()).all() and torch.isnan(f.qt_ms()).all() and torch.isnan(f.qtc_ms()).all()


# ------------------------------------------------------------------------------------------------ 3. inputs
def test_beats_of_the_detector_and_the_same_positions_as_lists_give_identical_tensors():
    from ecg_denoise_amd import BeatDetector
    x, _, _ = _records(3, 2, 3600, 24, 6.0)
    xd = torch.from_numpy(x).to(DEV)
    det = BeatDetector(device=DEV).detect(xd)
    assert min(len(p) for p in det.tolist()) >= 5
    a, _ = _delineate(xd, det)
    b, got = _delineate(xd, det.tolist())
    n = b.on.shape[1]
    assert n == max(det.count.tolist()) <= a.on.shape[1]
    for k in ("on", "off", "tpeak", "tend", "peaks"):
        assert torch.equal(getattr(a, k)[:, :n], getattr(b, k)) and (getattr(a, k)[:, n:] == -1).all(), k
    assert torch.equal(a.count, b.count)
    _against_oracle(x, det.tolist(), got)


def test_a_non_contiguous_fp64_input_equals_its_contiguous_fp32_copy():
    x, truth, _ = _records(3, 2, 3600, 24, 6.0)
    wide = torch.from_numpy(x).to(DEV).double().permute(0, 2, 1).contiguous().permute(0, 2, 1)      # (R, leads, T) over (R, T, leads)
    assert not wide.is_contiguous() and wide.dtype == torch.float64
    a, _ = _delineate(wide, truth)
    b, _ = _delineate(x, truth)
    assert _same(a, b)


def test_refusals_on_the_device():
    from ecg_denoise_amd import BeatDelineator, Beats, RalError
    dl = BeatDelineator(device=DEV)
    x = torch.zeros(2, 2, 1000, device=DEV)
    for beats in ([[5, 5], [1]], [[9, 3], [1]], [[1], [1000]], [[5]]):
        with pytest.raises(RalError, match="BeatDelineator.delineate"):
            dl.delineate(x, beats)
    with pytest.raises(RalError, match="1 beat lists on"):
        dl.delineate(x, Beats(torch.zeros(1, 4, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)))
    with pytest.raises(RalError, match="R <= 65535"):
        dl.delineate(torch.zeros(65536, 1, 8, device=DEV), [[1]] * 65536)


# ------------------------------------------------------------------------------------------------ 4. intervals
def test_intervals_are_the_formulas_on_the_device_integers():
    x, truth, _ = _records(3, 2, 3600, 24)
    for fs, q0 in ((360, 0.15), (500, 0.1)):
        f, got = _delineate(x, truth, fs=fs, q0=q0)
        on, off, tend, peaks = (t.cpu().numpy().astype(np.float64) for t in (f.on, f.off, f.tend, f.peaks))
        count = f.count.cpu().numpy()
        col = np.arange(on.shape[1])[None, :]
        qrs = np.where((on >= 0) & (off >= 0), (off - on) * 1000.0 / fs, np.nan)
        qt = np.where((on >= 0) & (tend >= 0), (tend - on) * 1000.0 / fs, np.nan)
        rr = np.full(on.shape, np.nan)
        rr[:, 1:] = np.where(col[:, 1:] < count[:, None], (peaks[:, 1:] - peaks[:, :-1]) / fs, np.nan)
        with np.errstate(invalid="ignore"):
            qtc = 1000.0 * (qt / 1000.0) / np.sqrt(rr)
        for name, want in (("qrs_ms", qrs), ("qt_ms", qt), ("qtc_ms", qtc)):
            mine = getattr(f, name)()
            assert mine.dtype == torch.float32 and mine.is_cuda and mine.shape == f.on.shape, name
            mine = mine.cpu().numpy().astype(np.float64)
            assert np.array_equal(np.isnan(mine), np.isnan(want)), name
            ok = ~np.isnan(want)
            assert ok.sum() >= 20 and np.all(np.abs(mine[ok] - want[ok]) <= RTOL * np.abs(want[ok])), name
        assert np.isnan(f.qtc_ms()[:, 0].cpu().numpy()).all()                # the first beat of a record has no RR before it
        assert np.array_equal(np.isnan(qrs), ~f.measurable()["qrs"].cpu().numpy())
        assert np.array_equal(np.isnan(qt), ~f.measurable()["qt"].cpu().numpy())
    assert 70.0 < np.nanmedian(qrs) * 500 / 360 < 130.0                       # (read at 360 Hz: a QRS duration)


# ------------------------------------------------------------------------------------------------ 5. composition
def _nan_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.isnan(a), torch.isnan(b)) and \
        torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0))


@pytest.mark.parametrize("fs", [360, 500])
def test_evaluate_intervals_is_the_explicit_composition(fs):
    """with a freshly initialised model: the plumbing, not an improvement (an untrained model promises none)"""
    from ecg_denoise_amd import (BeatDelineator, BeatDetector, ClassicalDenoiser, RateStreamingDenoiser, UNet, evaluate_intervals,
                                 mix_records, synth)
    from ecg_denoise_amd.infer import StreamingDenoiser
    model = UNet(leads=2, L=64, max_batch=16, train=False, device=DEV, seed=11).eval()
    T = 3600
    x, truth, _ = _records(3, 2, T, 24)
    rec = torch.from_numpy(x).to(DEV)
    noise = torch.from_numpy(synth.make_noise_record("ma", 2, T + 500, seed=3)).to(DEV)
    dn = StreamingDenoiser(model, use_graph=False) if fs == 360 else RateStreamingDenoiser(model, fs, use_graph=False)
    offs = [5, 200, 499]
    ev = evaluate_intervals(dn, rec, noise, 6.0, offsets=offs)
    noisy, clean = mix_records(rec, noise, 6.0, offsets=offs)
    ref = BeatDetector(fs, device=DEV).detect(clean)
    dl = BeatDelineator(fs, device=DEV)
    fc, fn, fd = dl.delineate(clean, ref), dl.delineate(noisy, ref), dl.delineate(dn.denoise(noisy), ref)
    assert ev.ref.tolist() == ref.tolist() and min(len(p) for p in ref.tolist()) >= 4
    assert _same(ev.clean, fc) and _same(ev.noisy, fn) and _same(ev.denoised, fd)
    for key, f in (("noisy", fn), ("denoised", fd)):
        for name, a, b, ms in (("qrs", "on", "off", "qrs_ms"), ("qt", "on", "tend", "qt_ms")):
            in_clean = (getattr(fc, a) >= 0) & (getattr(fc, b) >= 0)
            both = in_clean & (getattr(f, a) >= 0) & (getattr(f, b) >= 0)
            err = (getattr(f, ms)().double() - getattr(fc, ms)().double()).abs()
            err = torch.where(both, err, torch.zeros_like(err))
            assert _nan_equal(ev.share[key][name], both.sum(1).double() / in_clean.sum(1).double())
            assert _nan_equal(ev.mae_ms[key][name], err.sum(1) / both.sum(1).double())
            nb, nc = int(both.sum()), int(in_clean.sum())
            assert nc >= 6 and ev.pooled[key][name + "_beats"] == nb
            assert ev.pooled[key][name + "_share"] == nb / nc
            mae = ev.pooled[key][name + "_mae_ms"]           # (an untrained model may leave no beat measurable: NaN then)
            assert mae == float(err.sum()) / nb if nb else np.isnan(mae)
    if fs == 360:               # a reference given by the caller, per-record SNRs, and a classical denoiser in place of the model
        ev2 = evaluate_intervals(ClassicalDenoiser("fft", 1000, device=DEV), rec, noise, [0.0, 6.0, 12.0], ref=truth, offsets=offs)
        assert ev2.ref.tolist() == truth and set(ev2.pooled) == {"noisy", "denoised"}
        n2, c2 = mix_records(rec, noise, [0.0, 6.0, 12.0], offsets=offs)
        assert _same(ev2.clean, dl.delineate(c2, truth))
        assert _same(ev2.denoised, dl.delineate(ClassicalDenoiser("fft", 1000, device=DEV).denoise(n2), truth))
