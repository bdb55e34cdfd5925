"""Beat classes on the device: `BeatClassifier.classify` against the numpy oracle (tests/rhythm_util.py), `BeatClassPool` against
`classify` on the complete record bit for bit, and the composed `evaluate_rhythm` against its explicit composition.

Tolerances (rhythm_util): corr within 4 n 2^-24 absolute, n = leads (2 Wb + 1); rr_ratio within 4 * 2^-24 relative; labels equal
except where the oracle's corr or rr_ratio lies within its tolerance of its threshold, at most 1 % of the beats of a test
(tests/test_rhythm_cpu.py shows without a device that the synthetic records keep far from both thresholds)."""
import functools

import numpy as np
import pytest
import torch

import beat_util as B
import rhythm_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_MODELS = {}


@functools.lru_cache(maxsize=None)
def _records(R, leads, T, seed, db=None):
    """-> (float32 (R, leads, T), truth lists, truth labels): synthetic rhythm records, clean or with `emb` noise at `db` dB"""
    from ecg_denoise_amd import synth
    x, beats, labels = synth.make_records_with_rhythm(R, leads, T, seed=seed, p_v=0.12, p_s=0.08)
    if db is not None:
        z = synth.make_noise_record("emb", leads, T, seed=seed + 100).astype(np.float64)
        x = B.add_noise(x.astype(np.float64), z, db).astype(np.float32)
    return x, beats, labels


def _classify(x, beats, fs=360, **kw):
    """-> (BeatClasses, its tolist()) after the shape and padding checks"""
    from ecg_denoise_amd import BeatClassifier
    xd = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    c = BeatClassifier(fs, device=DEV, **kw).classify(xd, beats)
    R = 1 if xd.dim() == 2 else xd.shape[0]
    assert c.label.dtype == torch.int32 and c.corr.dtype == c.rr_ratio.dtype == torch.float32 and c.label.is_cuda
    assert c.label.shape == c.corr.shape == c.rr_ratio.shape == c.peaks.shape and c.label.shape[0] == R == len(c)
    for lab, co, rr, n in zip(c.label.tolist(), c.corr.tolist(), c.rr_ratio.tolist(), c.count.tolist()):
        assert all(v == -1 for v in lab[n:]) and all(np.isnan(v) for v in co[n:]) and all(np.isnan(v) for v in rr[n:])
    return c, c.tolist()


def _against_oracle(x, lists, got, fs=360, **kw):
    """every record against the oracle -> (beats compared, beats whose label was exempt)"""
    total = exempt = 0
    for r in range(len(lists)):
        exempt += U.compare(np.asarray(x[r], dtype=np.float64), lists[r], got[r], fs=fs, **kw)
        total += len(lists[r])
    assert exempt <= 0.01 * total, (exempt, total)
    return total, exempt


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _model():
    from ecg_denoise_amd import RALENet
    if "full" not in _MODELS:
        _MODELS["full"] = RALENet("full", leads=2, L=64, max_batch=16, train=False, device=DEV, seed=11).eval()
    return _MODELS["full"]


# ------------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("db", [None, 6.0])
def test_classify_equals_the_oracle_at_360_hz(db):
    """3 x 2 x 10 800, clean and with emb at 6 dB, at the detector's peaks and at the generator's own lists"""
    from ecg_denoise_amd import BeatDetector
    x, truth, labels = _records(3, 2, 10800, 11, db)
    xd = torch.from_numpy(x).to(DEV)
    det = BeatDetector(device=DEV).detect(xd)
    for beats, lists in ((det, det.tolist()), (truth, truth)):
        c, got = _classify(xd, beats)
        total, exempt = _against_oracle(x, lists, got)
        assert total >= 60 and min(len(p) for p in lists) >= 10
        cnt = c.counts().tolist()
        assert [sum(row) for row in cnt] == [len(p) for p in lists] and all(row[3] == 0 for row in cnt)
        assert [row[:3] for row in cnt] == [[g[0].count(k) for k in (0, 1, 2)] for g in got]
    if db is None:                         # at the true positions of clean records the classes are the generator's
        ext = 39
        for r in range(3):
            assert [l for l, p in zip(got[r][0], truth[r]) if ext <= p < 10800 - ext] == \
                   [l for l, p in zip(labels[r], truth[r]) if ext <= p < 10800 - ext]
        assert {l for row in labels for l in row} == {0, 1, 2}
    # other thresholds are honoured
    c, got = _classify(xd, truth, c0=0.5, r0=1.1)
    _against_oracle(x, truth, got, c0=0.5, r0=1.1)
    assert any(l == 2 for g in got for l in g[0])


def test_classify_equals_the_oracle_at_500_hz_with_12_leads():
    """2 x 12 x 15 000: the same samples read at 500 Hz (Wb = 50, Sa = 4: two rounds of the lane loop), 12 leads"""
    from ecg_denoise_amd import BeatDetector
    x, _, _ = _records(2, 12, 15000, 12)
    xd = torch.from_numpy(x).to(DEV)
    det = BeatDetector(fs=500, device=DEV).detect(xd)
    c, got = _classify(xd, det, fs=500)
    total, _ = _against_oracle(x, det.tolist(), got, fs=500)
    assert total >= 40
    c1, got1 = _classify(xd[1], [det.tolist()[1]], fs=500)                   # a single record, (leads, T), and a list
    assert torch.equal(_bits(c1.corr[0, :c1.count[0]]), _bits(c.corr[1, :c.count[1]])) and got1[0][0] == got[1][0]


# ------------------------------------------------------------------------------------------------ 2. short records, edges
def test_records_of_few_beats():
    """records of 1 440 samples hold 3 - 7 beats, so n <= K: every beat is judged among all the others"""
    x, truth, _ = _records(6, 2, 1440, 13)
    ns = sorted(len(t) for t in truth)
    assert 3 <= ns[0] and ns[-1] <= 7 and len(set(ns)) >= 3
    c, got = _classify(x, truth)
    _against_oracle(x, truth, got)
    for t, g in zip(truth, got):
        assert all(l == -1 for l in g[0]) if len(t) == 3 else all(l >= 0 for l in g[0])


def test_records_with_0_1_3_and_4_beats_and_beats_at_both_ends():
    x, _, _ = _records(6, 2, 1440, 13)
    T = x.shape[2]
    lists = [[], [100], [100, 400, 700], [100, 400, 700, 1000], [0, 300, 600, 900, T - 1], [0, 1, 2, T - 2, T - 1]]
    c, got = _classify(x, lists)
    assert c.count.tolist() == [0, 1, 3, 4, 5, 5] and tuple(c.label.shape) == (6, 5)
    _against_oracle(x, lists, got)
    assert got[0] == ([], [], []) and got[1][0] == [-1] and got[2][0] == [-1] * 3 and all(l >= 0 for l in got[3][0] + got[4][0])
    cnt = c.counts().tolist()
    assert cnt[:3] == [[0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 3]] and sum(cnt[3]) == 4 and cnt[3][3] == 0
    # a Beats with a wider cap than any count, as the detector gives
    from ecg_denoise_amd import Beats
    pad = torch.full((6, 40), -1, dtype=torch.int32, device=DEV)
    pad[:, :5] = c.peaks
    c2, got2 = _classify(x, Beats(pad, c.count))
    assert tuple(c2.label.shape) == (6, 40) and torch.equal(c2.label[:, :5], c.label)
    assert torch.equal(_bits(c2.corr[:, :5]), _bits(c.corr)) and torch.equal(_bits(c2.rr_ratio[:, :5]), _bits(c.rr_ratio))


def test_a_constant_record_has_correlation_zero():
    x = np.full((2, 2, 900), 3.0, dtype=np.float32)
    x[1] = 1024.0
    lists = [[100, 300, 500, 700], [50, 250, 450, 650, 850]]
    c, got = _classify(x, lists)
    assert got[0][1] == [0.0] * 4 and got[1][1] == [0.0] * 5 and got[0][0] == [1] * 4 and got[1][0] == [1] * 5
    assert np.isnan(got[0][2][0]) and got[0][2][1:] == [1.0, 1.0, 1.0]
    _against_oracle(x, lists, got)


def test_refusals():
    from ecg_denoise_amd import BeatClassifier, RalError
    cls = BeatClassifier(device=DEV)
    x = torch.zeros(2, 2, 1000, device=DEV)
    for beats in ([[5, 5]], [[5, 5], [1]], [[9, 3], [1]], [[-1], [1]], [[1], [1000]]):
        with pytest.raises(RalError):
            cls.classify(x, beats)
    with pytest.raises(RalError, match="device tensor"):
        cls.classify(torch.zeros(2, 2, 1000), [[1], [2]])
    with pytest.raises(RalError, match="not supported"):
        BeatClassifier(fs=4000, device=DEV).classify(x, [[1], [2]])
    with pytest.raises(RalError, match="R <= 65535"):
        cls.classify(torch.zeros(65536, 1, 8, device=DEV), [[1]] * 65536)


def test_beats_of_the_detector_and_the_same_positions_as_lists_give_identical_tensors():
    """2 x 2 x 3 600 at 360 Hz: a `Beats` (the detector's wider cap) against its own lists"""
    from ecg_denoise_amd import BeatDetector
    x, _, _ = _records(2, 2, 3600, 24)
    xd = torch.from_numpy(x).to(DEV)
    det = BeatDetector(device=DEV).detect(xd)
    assert min(len(p) for p in det.tolist()) >= 8
    a, _ = _classify(xd, det)
    b, _ = _classify(xd, det.tolist())
    n = b.label.shape[1]
    assert n == max(det.count.tolist()) < a.label.shape[1]
    for k in ("label", "corr", "rr_ratio", "peaks"):
        assert torch.equal(_bits(getattr(a, k)[:, :n]), _bits(getattr(b, k))), k
    assert (a.label[:, n:] == -1).all() and (a.peaks[:, n:] == -1).all() and torch.equal(a.count, b.count)
    assert torch.isnan(a.corr[:, n:]).all() and torch.isnan(a.rr_ratio[:, n:]).all()


# ------------------------------------------------------------------------------------------------ 3. pool equals record
def _whole(rec, fs=360):
    """the complete record through detect and classify -> (peaks, label, corr bits, rr bits) as lists"""
    from ecg_denoise_amd import BeatClassifier, BeatDetector
    beats = BeatDetector(fs, device=DEV).detect(rec)
    c = BeatClassifier(fs, device=DEV).classify(rec, beats)
    n = int(c.count[0])
    return [beats.peaks[0, :n].tolist(), c.label[0, :n].tolist(), _bits(c.corr[0, :n]).tolist(), _bits(c.rr_ratio[0, :n]).tolist()]


def _add(acc, res):
    peaks, label, corr, rr = res
    assert peaks.dtype == torch.int64 and label.dtype == torch.int32 and corr.dtype == rr.dtype == torch.float32 and peaks.is_cuda
    assert peaks.shape == label.shape == corr.shape == rr.shape and peaks.dim() == 1
    for a, t in zip(acc, (peaks, label, _bits(corr), _bits(rr))):
        a += t.tolist()
    return peaks.numel()


def test_pool_equals_classify_on_the_complete_record():
    """three streams through two slots (the third reuses the slot of the short one, which closes before its ninth beat),
    opened at different calls, in random chunks of 1 .. 4 000 samples"""
    from ecg_denoise_amd import BeatClassPool
    x, _, _ = _records(3, 2, 10800, 11, 6.0)
    cuts = [10800, 1440, 9000]
    recs = [torch.from_numpy(np.ascontiguousarray(r[:, :T])).to(DEV) for r, T in zip(x, cuts)]
    want = [_whole(r) for r in recs]
    assert len(want[0][0]) > 20 and 3 < len(want[1][0]) < 9 and len(want[2][0]) > 20
    pool = BeatClassPool(2, capacity=2, device=DEV)
    rng = np.random.default_rng(7)
    sid, pos, got, done = {}, {}, [[[], [], [], []] for _ in recs], set()
    call, first_out = 0, {}
    while len(done) < 3:
        for i in range(3):
            if i not in sid and call >= 2 * i and len(pool.open_streams) < pool.capacity:
                sid[i], pos[i] = pool.open(), 0
        chunks, close = {}, []
        for i in list(sid):
            if i in done or rng.random() < 0.3:
                continue
            c = min(cuts[i] - pos[i], int(rng.integers(1, 4001)))
            if pos[i] + c == cuts[i]:
                close.append(sid[i])
            chunks[sid[i]] = recs[i][:, pos[i]:pos[i] + c]
        call += 1
        if not chunks:
            continue
        res = pool.push(chunks, close=close)
        assert set(res) == set(chunks)
        for i in list(sid):
            if i not in done and sid[i] in res:
                pos[i] += chunks[sid[i]].shape[1]
                n = _add(got[i], res[sid[i]])
                if n and i not in first_out:
                    first_out[i] = n
                if sid[i] in close:
                    done.add(i)
    assert got == want
    assert sid[2] == sid[1] and first_out[1] == len(want[1][0]) and first_out[0] >= 9 and first_out[2] >= 9
    assert pool.open_streams == ()


def test_pool_one_sample_at_a_time_then_a_chunk_of_many_beats_alone_in_the_pool():
    from ecg_denoise_amd import BeatClassPool
    x, _, _ = _records(3, 2, 10800, 11)
    rec = torch.from_numpy(x[2]).to(DEV)
    want = _whole(rec)
    pool = BeatClassPool(2, capacity=1, device=DEV)
    a = pool.open()
    got = [[], [], [], []]
    for t in range(2000):
        assert _add(got, pool.push({a: rec[:, t:t + 1]})[a]) == 0          # fewer than nine beats so far: nothing is final
    before = pool.beats_in(a)
    assert 0 < before < 9 and pool.samples_in(a) == 2000
    n = _add(got, pool.push({a: rec[:, 2000:9000]})[a])                    # one chunk, more than K new beats
    assert pool.beats_in(a) - before > 8 and n == pool.beats_in(a)
    for t in range(9000, 9400):                                            # every later beat comes out with the push that detects it
        k = pool.beats_in(a)
        assert _add(got, pool.push({a: rec[:, t:t + 1]})[a]) == pool.beats_in(a) - k
    _add(got, pool.close(a, rec[:, 9400:]))
    assert got == want
    # the slot again, for a stream that ends with three beats: unclassified, as in the record
    b = pool.open()
    assert b == a
    short = rec[:, 3000:3000 + 900]
    w = _whole(short)
    g = [[], [], [], []]
    _add(g, pool.push({b: short[:, :500]})[b])
    _add(g, pool.close(b, short[:, 500:]))
    assert g == w and 1 <= len(w[0]) <= 4


def test_pool_raising_calls_change_nothing():
    """a pool that is given bad calls between its pushes gives what an undisturbed twin gives"""
    from ecg_denoise_amd import BeatClassPool, RalError
    x, _, _ = _records(3, 2, 10800, 11)
    recs = [torch.from_numpy(r).to(DEV) for r in x[:2]]
    pools = [BeatClassPool(2, capacity=3, device=DEV) for _ in range(2)]
    ids = [(p.open(), p.open()) for p in pools]
    assert ids[0] == ids[1]
    a, b = ids[0]
    outs = [[[[], [], [], []] for _ in range(2)] for _ in range(2)]
    steps = [(0, 700), (700, 2500), (2500, 2501), (2501, 6000), (6000, 10800)]
    for k, (lo, hi) in enumerate(steps):
        p = pools[0]
        snap = (p.ring.clone(), p.ring_pos.clone(), p.beats.hist.clone(), p.state.nb.copy(), p.state.done.copy(), p.beats.state.n.copy(),
                p.beats.state.turn.copy())
        for chunks, close in (({a: recs[0][:, :10], 2: recs[0][:, :10]}, ()),        # slot 2 holds no open stream
                              ({a: recs[0][:, :10], b: recs[0][:1, :10]}, ()),       # wrong number of leads
                              ({a: recs[0][0, :10]}, ()), ({a: recs[0][:, :10]}, (7,)), ({}, ())):
            with pytest.raises(RalError):
                p.push(chunks, close=close)
        c = p.open()
        with pytest.raises(RalError, match="without a single sample"):
            p.push({a: recs[0][:, :10]}, close=(c,))
        p.beats.state.is_open[c] = False
        p.beats.state.free.append(c)
        now = (p.ring, p.ring_pos, p.beats.hist, p.state.nb, p.state.done, p.beats.state.n, p.beats.state.turn)
        assert all(torch.equal(u, v) if torch.is_tensor(u) else np.array_equal(u, v) for u, v in zip(snap, now))
        for q, pool in enumerate(pools):
            res = pool.push({a: recs[0][:, lo:hi], b: recs[1][:, lo:hi]}, close=(a, b) if hi == 10800 else ())
            _add(outs[q][0], res[a])
            _add(outs[q][1], res[b])
    assert outs[0] == outs[1] == [_whole(r) for r in recs]


# ------------------------------------------------------------------------------------------------ 4. composition
@pytest.mark.parametrize("fs", [360, 500])
def test_evaluate_rhythm_is_the_explicit_composition(fs):
    """with a freshly initialised model: the plumbing, not an improvement (an untrained model promises none)"""
    from ecg_denoise_amd import (BeatClassifier, BeatDetector, RateStreamingDenoiser, evaluate_rhythm, mix_records, scoring,
                                 synth)
    from ecg_denoise_amd.infer import StreamingDenoiser
    model = _model()
    T = 6000
    x, truth, labels = _records(3, 2, T, 14)
    rec = torch.from_numpy(x).to(DEV)
    noise = torch.from_numpy(synth.make_noise_record("emb", 2, T + 500, seed=3)).to(DEV)
    dn = StreamingDenoiser(model, use_graph=False) if fs == 360 else RateStreamingDenoiser(model, fs, use_graph=False)
    ev = evaluate_rhythm(dn, rec, noise, 0.0, offsets=[5, 200, 499])
    noisy, clean = mix_records(rec, noise, 0.0, offsets=[5, 200, 499])
    ref = BeatDetector(fs, device=DEV).detect(clean)
    cls = BeatClassifier(fs, device=DEV)
    c0, c1, c2 = cls.classify(clean, ref), cls.classify(noisy, ref), cls.classify(dn.denoise(noisy), ref)
    assert ev.ref.tolist() == ref.tolist() and min(len(p) for p in ref.tolist()) >= 9
    for mine, theirs in ((ev.clean, c0), (ev.noisy, c1), (ev.denoised, c2)):
        assert torch.equal(mine.label, theirs.label) and torch.equal(_bits(mine.corr), _bits(theirs.corr))
        assert torch.equal(_bits(mine.rr_ratio), _bits(theirs.rr_ratio))
    mask = (c0.label >= 0) & (c1.label >= 0) & (c2.label >= 0)
    truth_v = (c0.label[mask] == 1).long()
    assert torch.equal(ev.mask, mask) and torch.equal(ev.truth, truth_v) and int(mask.sum()) >= 27
    for name, c in (("noisy", c1), ("denoised", c2)):
        lg = c.logits(mask)[0]
        for key, fn in (("acc", scoring.acc), ("precision", scoring.precision), ("f1", scoring.f1_score)):
            try:
                want = fn(lg, truth_v)
            except ZeroDivisionError:
                want = float("nan")
            assert ev.scores[name][key] == want or (np.isnan(want) and np.isnan(ev.scores[name][key]))
    if fs == 360:                   # a reference and its labels given by the caller: the generator's
        ev2 = evaluate_rhythm(dn, rec, noise, [0.0, 6.0, 12.0], ref=truth, ref_labels=labels, offsets=[5, 200, 499])
        assert ev2.ref.tolist() == truth
        want = torch.tensor([l for row, m in zip(labels, ev2.mask.tolist()) for l, keep in zip(row, m) if keep], device=DEV)
        assert torch.equal(ev2.truth, (want == 1).long()) and set(ev2.scores) == {"noisy", "denoised"}


def test_logits_reproduce_the_counts_of_the_labels():
    from ecg_denoise_amd import scoring
    x, truth, labels = _records(3, 2, 10800, 11, 6.0)
    c, got = _classify(x, truth)
    lg, sel = c.logits()
    assert lg.dtype == torch.float32 and tuple(lg.shape) == (int(sel.sum()), 2) and torch.equal(sel, c.label >= 0)
    said_v = torch.tensor([l == 1 for g in got for l in g[0] if l >= 0], device=DEV)
    assert torch.equal(torch.argmax(lg, dim=1) == 1, said_v)
    true_v = torch.tensor([int(l == 1) for row, g in zip(labels, got) for l, k in zip(row, g[0]) if k >= 0], device=DEV)
    tp = int((said_v & (true_v == 1)).sum())
    fp = int((said_v & (true_v == 0)).sum())
    fn = int((~said_v & (true_v == 1)).sum())
    tn = int((~said_v & (true_v == 0)).sum())
    assert tp >= 5 and tn >= 50
    assert scoring.confusion(lg, true_v) == (tp, fp, fn, tn)
    assert scoring.acc(lg, true_v) == (tp + tn) / len(true_v) and scoring.precision(lg, true_v) == tp / (tp + fp)
    assert scoring.f1_score(lg, true_v) == tp / (tp + 0.5 * (fp + fn))
