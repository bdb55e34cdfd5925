"""Beat detection on the device: `BeatDetector.detect` against the numpy oracle integer for integer, `BeatPool` against `detect`
on the complete record, `match_beats` against the numpy walk, and the composed `evaluate_beats` against its explicit composition.

Exact comparison with an fp64 oracle is legitimate only where no decision of the record lies near a tie; `_oracle` asserts the
oracle's three margins (tests/test_beats_cpu.py does the same for the shared inputs, without a device) before anything is
compared: threshold 1e-2, top of f 1e-5, 2 samples from the window edge - three orders above fp32 rounding."""
import numpy as np
import pytest
import torch

import beat_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGINS = {"threshold": 1e-2, "top": 1e-5, "edge": 2}
_MODELS = {}


def _oracle(x, **kw):
    """x (R, leads, T) -> the oracle's lists, after the guard"""
    out = []
    for r in np.asarray(x):
        peaks, mg = U.detect(r, margins=True, **kw)
        assert all(mg[k] >= MARGINS[k] for k in MARGINS), mg
        out.append(peaks)
    return out


def _detect(x, **kw):
    from ecg_denoise_amd import BeatDetector
    x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    det = BeatDetector(device=DEV, **kw)
    b = det.detect(x.to(DEV))
    R, T = (1 if x.dim() == 2 else x.shape[0]), x.shape[-1]
    assert b.peaks.dtype == torch.int32 and tuple(b.peaks.shape) == (R, T // (det.geometry["Rf"] + 1) + 1) and b.peaks.is_cuda
    lists = b.tolist()
    for row, n, p in zip(b.peaks.tolist(), b.count.tolist(), lists):
        assert n <= len(row) and row[:n] == p and all(v == -1 for v in row[n:]) and p == sorted(set(p))
    return lists


def _model():
    from ecg_denoise_amd import RALENet
    if "full" not in _MODELS:
        _MODELS["full"] = RALENet("full", leads=2, L=64, max_batch=16, train=False, device=DEV, seed=11).eval()
    return _MODELS["full"]


# ------------------------------------------------------------------------------------------------ 1. against the oracle
def test_detect_equals_the_oracle_on_the_shared_inputs():
    """the 30 records of beat_util.inputs(): clean, emb at 6 dB and at 0 dB"""
    want = U.expected()
    n = 0
    for name, x in U.inputs():
        assert _detect(x) == want[name], name
        n += len(x)
        assert all(len(p) >= 3 for p in want[name]), name          # (records with beats, not empty lists that agree)
    assert n == 30


def test_detect_equals_the_oracle_at_500_hz_and_with_12_leads():
    from ecg_denoise_amd import Resampler, synth
    x = dict(U.inputs())["seed7_3x2x3000_emb6dB"]
    x500 = Resampler(360, 500, DEV).convert(torch.from_numpy(x)).cpu().numpy()
    assert x500.shape == (3, 2, 4167)
    assert _detect(x500, fs=500) == _oracle(x500, fs=500)
    x12 = U.zscore(synth.make_records(2, 12, 1440, seed=8)).astype(np.float32)
    assert _detect(x12) == _oracle(x12)
    assert _detect(x12[0]) == _oracle(x12[:1])                       # a single record, (leads, T)
    other = dict(alpha=0.5, band=(5, 30))                            # another threshold and band
    assert _detect(x, **other) == _oracle(x, **other)


# ------------------------------------------------------------------------------------------------ 2. against the truth
@pytest.mark.parametrize("T", [1440, 2000])
def test_clean_synthetic_records_give_every_true_beat(T):
    """single-strip records whose true beats lie more than Rf apart: Se = +P = 1 at 150 ms, every detection within 2 samples"""
    from ecg_denoise_amd import BeatDetector, beat_geometry, match_beats, synth
    x, truth = synth.make_records_with_beats(4, 2, T, seed=5)
    assert min(np.diff(t).min() for t in truth) > beat_geometry(360)["Rf"]
    b = BeatDetector(device=DEV).detect(torch.from_numpy(x).to(DEV))
    sc = match_beats(truth, b)
    total = sum(len(t) for t in truth)
    assert sc.tp.tolist() == [len(t) for t in truth] and sc.pooled["tp"] == total and sc.pooled["fp"] == sc.pooled["fn"] == 0
    assert sc.pooled["sensitivity"] == sc.pooled["ppv"] == sc.pooled["f1"] == 1.0
    assert torch.equal(sc.sensitivity, torch.ones(4, dtype=torch.float64, device=DEV)) and torch.equal(sc.ppv, sc.f1)
    assert max(abs(p - t) for ps, ts in zip(b.tolist(), truth) for p, t in zip(ps, ts)) <= 2
    rr = b.rr_seconds()
    assert len(rr) == 4 and all(len(r) == len(t) - 1 and np.all((r > 0.2) & (r < 1.5)) for r, t in zip(rr, truth))


# ------------------------------------------------------------------------------------------------ 3. edge cases
def test_records_shorter_than_every_window():
    x = dict(U.inputs())["seed5_4x2x1440_clean"]
    for T in (16, 100):
        for start in (0, 700):
            cut = np.ascontiguousarray(x[:, :, start:start + T])
            assert _detect(cut) == _oracle(cut), (T, start)
    assert _detect(x[:, :, 5:6]) == _oracle(x[:, :, 5:6]) == [[0]] * 4     # T = 1


def test_constant_records_and_a_record_of_one_beat():
    """an exactly silent record has no peak; a constant one has none above a floor (without one its rounding residue is its
    signal: the header says so); one R wave gives one peak, at its top"""
    assert _detect(np.zeros((2, 2, 1500), dtype=np.float32)) == [[], []]
    assert _detect(np.full((2, 2, 1500), 1024.0, dtype=np.float32), floor=1e-6) == [[], []]
    t = np.arange(1200, dtype=np.float64)
    one = np.stack([np.exp(-0.5 * ((t - 611) / 4.0) ** 2), 0.6 * np.exp(-0.5 * ((t - 611) / 4.7) ** 2)])[None].astype(np.float32)
    assert _detect(one) == _oracle(one) == [[611]]
    assert _detect(one + 1024.0, floor=1e-6) == [[611]]                   # on an ADC baseline


def test_grid_limit_and_refusals():
    from ecg_denoise_amd import BeatDetector, RalError
    det = BeatDetector(device=DEV)
    x = torch.zeros(65535, 1, 16, device=DEV)
    x[-1, 0, 8] = 1.0
    b = det.detect(x)
    assert tuple(b.peaks.shape) == (65535, 1) and int(b.count.sum()) == 1 and b.peaks[-1].tolist() == [8]
    with pytest.raises(RalError, match="R <= 65535"):
        det.detect(torch.zeros(65536, 1, 16, device=DEV))
    with pytest.raises(RalError, match="not supported"):
        det.detect(torch.zeros(1, 52, 2000, device=DEV))                  # the spans of 52 leads do not fit
    with pytest.raises(RalError, match="not supported"):
        BeatDetector(fs=2000, device=DEV).detect(torch.zeros(1, 2, 9000, device=DEV))
    with pytest.raises(RalError, match="device tensor"):
        det.detect(torch.zeros(1, 2, 2000))
    with pytest.raises(RalError):
        det.detect(torch.zeros(2, 0, device=DEV))


# ------------------------------------------------------------------------------------------------ 4. pool equals record
def _run_pool(pool, recs, rng, chunk_sizes, stagger=2, omit=0.3):
    """feed the records through a pool, one stream each, opened at different calls, in random chunks -> per record its peaks;
    checks after every call that the peaks given are new, ascending and decided"""
    from ecg_denoise_amd import beat_frontier
    n_streams = len(recs)
    sid, pos, outs, done = {}, {}, {i: [] for i in range(n_streams)}, set()
    call = 0
    while len(done) < n_streams:
        for i in range(n_streams):
            if i not in sid and call >= stagger * i and len(pool.open_streams) < pool.capacity:
                sid[i], pos[i] = pool.open(), 0
                pool.hist[:, sid[i]].fill_(float("nan"))         # a slot, fresh or reused: nothing before sample 0 may be read
        chunks, close = {}, []
        for i in list(sid):
            if i in done or rng.random() < omit:
                continue
            T = recs[i].shape[1]
            c = min(T - pos[i], int(rng.choice(chunk_sizes)))
            if pos[i] + c == T:
                close.append(sid[i])
                if c and rng.random() < 0.5:       # the last samples now, the close without a chunk in the next call
                    close.pop()
            if c:
                chunks[sid[i]] = recs[i][:, pos[i]:pos[i] + c]
        call += 1
        if not chunks and not close:
            continue
        res = pool.push(chunks, close=close)
        assert set(res) == set(chunks) | set(close)
        for i in list(sid):
            if i not in done and sid[i] in res:
                pos[i] += chunks[sid[i]].shape[1] if sid[i] in chunks else 0
                got = res[sid[i]]
                assert got.dtype == torch.int64 and got.is_cuda and got.dim() == 1
                outs[i] += got.tolist()
                if sid[i] in close:
                    done.add(i)
                else:
                    assert all(p < beat_frontier(pos[i], pool.fs) + pool.geometry["Rw"] for p in outs[i])
    return [outs[i] for i in range(n_streams)]


@pytest.mark.parametrize("name,fs", [("seed7_3x2x3000_emb6dB", 360), ("seed6_3x1x2000_emb0dB", 360), ("seed5_4x2x1440_clean", 250)])
def test_pool_equals_detect_on_the_complete_record(name, fs):
    """ragged chunks (one-sample chunks among them), streams that open and close mid-way through three slots, records of
    different lengths; at 250 Hz the same samples are simply read at another rate"""
    from ecg_denoise_amd import BeatPool
    x = dict(U.inputs())[name]
    cuts = [x.shape[2], x.shape[2] - 301, 777, x.shape[2] - 1][:len(x)]
    recs = [torch.from_numpy(np.ascontiguousarray(r[:, :T])).to(DEV) for r, T in zip(x, cuts)]
    want = [_detect(r, fs=fs)[0] for r in recs]
    assert sum(len(w) for w in want) >= 10
    pool = BeatPool(x.shape[1], capacity=3 if len(x) > 3 else 2, fs=fs, device=DEV)
    rng = np.random.default_rng(len(name) + fs)
    got = _run_pool(pool, recs, rng, [1, 1, 2, 33, 360, 700, 2500])
    assert got == want
    assert pool.open_streams == ()


def test_pool_one_sample_chunks_a_stream_alone_and_a_short_stream():
    from ecg_denoise_amd import BeatPool, beat_frontier
    x = dict(U.inputs())["seed5_4x2x1440_emb6dB"]
    rec = torch.from_numpy(np.ascontiguousarray(x[1][:, :1000])).to(DEV)
    want = _detect(rec)[0]
    pool = BeatPool(2, capacity=2, device=DEV)
    a = pool.open()
    got = []
    for t in range(1000):                                            # sample by sample, from the first to the last
        got += pool.push({a: rec[:, t:t + 1]})[a].tolist()
        assert pool.samples_in(a) == t + 1
    mid = len(got)
    got += pool.close(a).tolist()
    assert got == want and 0 < mid < len(want) and beat_frontier(1000) == 343
    # a stream closed while shorter than half (90 samples), beside one that goes on
    a, b = pool.open(), pool.open()
    ga = pool.push({a: rec[:, :800], b: rec[:, 100:140]})[a].tolist()
    short = pool.push({a: rec[:, 800:900]}, close=(b,))
    assert short[b].tolist() == _detect(rec[:, 100:140])[0]
    ga += short[a].tolist() + pool.close(a, rec[:, 900:]).tolist()
    assert ga == want


def test_pool_history_planes_hold_the_last_samples_received():
    """the history itself (tests/slot_util.py): chunks around hist_len = 1314, a slot reused after both its planes were set to
    NaN; and the peaks of all four streams still equal the record path's"""
    from slot_util import run_with_history_checks
    from ecg_denoise_amd import BeatPool
    pool = BeatPool(2, 3, 360, device=DEV)
    assert pool.hist_len == 1314
    x = dict(U.inputs())["seed7_3x2x3000_emb6dB"]
    long = np.concatenate([x[0], x[1]], axis=1)                      # (2, 6000)
    recs = [torch.from_numpy(np.ascontiguousarray(r)).to(DEV) for r in (long[:, :4100], long[:, 1000:1000 + 3943], long[:, 1500:5500],
                                                                        x[2][:, :1400])]
    want = [_detect(r)[0] for r in recs]
    assert sum(len(w) for w in want) >= 10
    got = [torch.cat(outs).tolist() for outs in run_with_history_checks(pool, recs)]
    assert got == want


def test_pool_raising_calls_change_nothing():
    from ecg_denoise_amd import BeatPool, RalError, _lib
    from ecg_denoise_amd.model import _ptr, _stream
    pool = BeatPool(2, capacity=3, device=DEV)
    a, b = pool.open(), pool.open()
    x = torch.from_numpy(dict(U.inputs())["seed7_3x2x3000_clean"][0])
    pool.push({a: x[:, :900], b: x[:, :37]})
    snap = lambda: (pool.hist.clone(), pool.state.n.copy(), pool.state.turn.copy(), pool.state.is_open.copy(), list(pool.state.free))
    before = snap()

    def unchanged():
        now = snap()
        assert torch.equal(now[0], before[0]) and all(np.array_equal(p, q) for p, q in zip(now[1:], before[1:]))

    for chunks, close in (({a: x[:, :10], 2: x[:, :10]}, ()),           # slot 2 holds no open stream
                          ({a: x[:, :10], b: x[:1, :10]}, ()),          # wrong number of leads
                          ({a: x[:, :10], b: x[0, :10]}, ()),
                          ({a: x[:, :10]}, (7,)),
                          ({}, ())):
        with pytest.raises(RalError):
            pool.push(chunks, close=close)
        unchanged()
    c = pool.open()
    with pytest.raises(RalError, match="without a single sample"):
        pool.push({a: x[:, :10]}, close=(c,))
    pool.state.is_open[c] = False
    pool.state.free.append(c)
    unchanged()
    # the entry point checks the host table before it launches anything
    sids, tab = pool.plan({a: (2, 500), b: (2, 50)})
    d, lib = pool.det, _lib.lib()
    xp = torch.zeros(550 * 2, device=DEV)
    peaks = torch.zeros(max(int(tab["cap"].sum()), 1), dtype=torch.int64, device=DEV)
    count = torch.zeros(2, dtype=torch.int32, device=DEV)
    tab_dev = torch.empty(len(tab) * tab.itemsize, dtype=torch.uint8, device=DEV)
    nbytes = lib.ral_beat_records_scratch_bytes(2, 2, pool.state.span(tab), d.geom)
    scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=DEV)

    def call(t, x_total=550, hist_len=None, scratch_bytes=None, ntaps=None):
        return lib.ral_beat_pool(_ptr(pool.hist), _ptr(xp), x_total, t.ctypes.data, len(t), _ptr(tab_dev), 1, pool.capacity, 2,
                                 d.geom, _ptr(d.bank), d.bank_host.size if ntaps is None else ntaps,
                                 pool.hist_len if hist_len is None else hist_len, _ptr(scratch),
                                 scratch.numel() * 8 if scratch_bytes is None else scratch_bytes, _ptr(peaks),
                                 int(tab["cap"].sum()), _ptr(count), _stream())

    def broken(field, row, value):
        t = tab.copy()
        t[field][row] = value
        return t

    assert int(tab["d"][0]) == 500 and int(tab["d"][1]) == 0
    for t, kw, rule in ((broken("slot", 1, 3), {}, "0 <= slot < capacity"),
                        (broken("slot", 1, int(tab["slot"][0])), {}, "every slot at most once"),
                        (broken("x_off", 1, 501), {}, "the chunk inside the packed chunks"),
                        (broken("out_off", 0, 1), {}, "the row's peaks inside the packed peaks"),
                        (broken("d", 0, 501), {}, "decisions that are final"),
                        (broken("cap", 0, 2), {}, "cap >= ceil"),
                        (broken("n0", 0, int(tab["n0"][0]) + 5000), {}, "decisions that are final|inside the history"),
                        (broken("turn", 0, 2), {}, "turn 0 or 1"),
                        (broken("T", 0, 5), {}, "T = n0 \\+ c"),
                        (tab, {"hist_len": pool.hist_len - 1}, "hist_len >= 2"),
                        (tab, {"scratch_bytes": 64}, "scratch"),
                        (tab, {"ntaps": 180}, "ntaps = 2 half \\+ 1")):
        assert call(t, **kw) != 0
        msg = lib.ral_last_error().decode()
        assert msg.startswith("beat_pool: need ") and __import__("re").search(rule, msg), msg
        unchanged()
    assert call(tab) == 0                      # the sound table runs
    torch.cuda.synchronize()
    assert count.tolist()[1] == 0


# ------------------------------------------------------------------------------------------------ 5. composition
@pytest.mark.parametrize("fs", [360, 500])
def test_beat_pool_behind_a_live_pool(fs):
    """whatever each push of the denoising pool returns goes into the BeatPool; the peaks equal `detect` on the concatenation
    of those same chunks (`RateLivePool` at 500 Hz, `LivePool` at 360)"""
    from ecg_denoise_amd import BeatPool, LivePool, RateLivePool
    model = _model()
    T = 2600 if fs == 360 else 3600
    x = U.zscore(__import__("ecg_denoise_amd").synth.make_records(2, 2, T, seed=9)).astype(np.float32)
    recs = [torch.from_numpy(r).to(DEV) for r in x]
    live = LivePool(model, capacity=2) if fs == 360 else RateLivePool(model, fs, capacity=2)
    beats = BeatPool(2, capacity=2, fs=fs, device=DEV)
    ls, bs = [live.open() for _ in recs], [beats.open() for _ in recs]
    rng = np.random.default_rng(fs)
    pos, den, got = [0, 0], [[], []], [[], []]
    while any(s is not None for s in ls):
        chunks, close = {}, []
        for i, r in enumerate(recs):
            if ls[i] is None:
                continue
            c = min(T - pos[i], int(rng.choice([1, 50, 360, 900])))
            chunks[ls[i]] = r[:, pos[i]:pos[i] + c]
            pos[i] += c
            if pos[i] == T:
                close.append(ls[i])
        out = live.push(chunks, close=close)
        fed = {bs[i]: out[ls[i]] for i in range(2) if ls[i] in out}
        res = beats.push(fed, close=[bs[i] for i in range(2) if ls[i] in close])
        for i in range(2):
            if ls[i] in out:
                den[i].append(out[ls[i]])
                got[i] += res[bs[i]].tolist()
                if ls[i] in close:
                    ls[i] = None
    for i in range(2):
        whole = torch.cat(den[i], dim=1)
        assert whole.shape[1] == T
        assert got[i] == _detect(whole, fs=fs)[0] and len(got[i]) >= 3


# ------------------------------------------------------------------------------------------------ 6. matching
def test_match_beats_equals_the_numpy_walk():
    from ecg_denoise_amd import RalError, match_beats
    cases = [([], []), ([], [5, 900]), ([100, 400], []), ([100], [154]), ([100], [155]), ([154], [100]), ([155], [100]),
             ([100, 200, 300], [100, 200, 300]), ([100, 200, 300], [40, 110, 150, 290, 1000]),
             ([10, 20, 30, 1000], [70, 80, 2000]), ([500, 560], [530]), ([530], [476, 584]), ([0], [54]), ([0, 2 ** 31 - 1], [2 ** 31 - 56])]
    ref, det = [c[0] for c in cases], [c[1] for c in cases]
    sc = match_beats(ref, det, device=DEV)
    assert sc.tol == 54
    want = [U.match(r, d, 54) for r, d in cases]
    assert [tuple(v) for v in sc.counts.tolist()] == want
    assert want[3] == (1, 0, 0) and want[4] == (0, 1, 1) and want[1] == (0, 2, 0) and want[2] == (0, 0, 2)     # ties at tol, all FP, all FN
    tot = np.sum(want, axis=0)
    assert (sc.pooled["tp"], sc.pooled["fp"], sc.pooled["fn"]) == tuple(tot)
    assert sc.pooled["sensitivity"] == tot[0] / (tot[0] + tot[2]) and sc.pooled["ppv"] == tot[0] / (tot[0] + tot[1])
    assert torch.isnan(sc.sensitivity[0]) and torch.isnan(sc.ppv[0]) and sc.f1[7].item() == 1.0
    for tol_s, fs in ((0.0, 360), (0.15, 500), (1.0, 250)):
        sc = match_beats(ref, [torch.tensor(d) for d in det], tol_s=tol_s, fs=fs, device=DEV)
        assert [tuple(v) for v in sc.counts.tolist()] == [U.match(r, d, int(tol_s * fs)) for r, d in cases]
    with pytest.raises(RalError):
        match_beats([[1, 2]], [[1], [2]], device=DEV)
    with pytest.raises(RalError, match="ascending"):
        match_beats([[5, 2]], [[1]], device=DEV)


# ------------------------------------------------------------------------------------------------ 7. evaluate_beats
@pytest.mark.parametrize("fs", [360, 500])
def test_evaluate_beats_is_the_explicit_composition(fs):
    """with a freshly initialised model: the plumbing, not an improvement (an untrained model promises none)"""
    from ecg_denoise_amd import BeatDetector, RateStreamingDenoiser, evaluate_beats, match_beats, mix_records, synth
    from ecg_denoise_amd.infer import StreamingDenoiser
    model = _model()
    T = 2600 if fs == 360 else 3600
    rec = torch.from_numpy(synth.make_records(3, 2, T, seed=4)).to(DEV)
    noise = torch.from_numpy(synth.make_noise_record("emb", 2, T + 500, seed=3)).to(DEV)
    dn = StreamingDenoiser(model, use_graph=False) if fs == 360 else RateStreamingDenoiser(model, fs, use_graph=False)
    ev = evaluate_beats(dn, rec, noise, -4.0, offsets=[5, 200, 499])
    noisy, clean = mix_records(rec, noise, -4.0, offsets=[5, 200, 499])
    det = BeatDetector(fs, device=DEV)
    ref, bn, bd = det.detect(clean), det.detect(noisy), det.detect(dn.denoise(noisy))
    assert ev.ref.tolist() == ref.tolist() and ev.det_noisy.tolist() == bn.tolist() and ev.det_denoised.tolist() == bd.tolist()
    assert torch.equal(ev.noisy.counts, match_beats(ref, bn, fs=fs).counts)
    assert torch.equal(ev.denoised.counts, match_beats(ref, bd, fs=fs).counts)
    n_ref = [len(r) for r in ref.tolist()]
    assert min(n_ref) >= 3
    for sc in (ev.noisy, ev.denoised):
        assert (sc.tp + sc.fn).tolist() == n_ref
        assert set(sc.pooled) == {"tp", "fp", "fn", "sensitivity", "ppv", "f1"}
        assert sc.sensitivity.shape == sc.ppv.shape == sc.f1.shape == (3,)
    # a reference given by the caller
    truth = [[100, 700, 1500]] * 3
    ev2 = evaluate_beats(dn, rec, noise, [-4.0, 0.0, 4.0], ref=truth, offsets=[5, 200, 499])
    assert (ev2.noisy.tp + ev2.noisy.fn).tolist() == [3, 3, 3] and (ev2.denoised.tp + ev2.denoised.fn).tolist() == [3, 3, 3]
