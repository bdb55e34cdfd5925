"""Sample-rate conversion on the device: `Resampler` against scipy's recorded results, `ResamplerPool` against `Resampler`
bit for bit, calls that raise, and the composed `RateStreamingDenoiser` / `RateLivePool` against their explicit compositions."""
import os

import numpy as np
import pytest
import torch

import rate_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g9_rate.npz")
_MODELS = {}


def _model(kind):
    """one eval-mode model per kind for the module: the 2-lead RA-LENet and the 12-lead NewRALE of the pool tests (and a 2-lead
    one with L = 128, for an overlap of 64 samples)"""
    from ecg_denoise_amd import NewRALE, RALENet
    if kind not in _MODELS:
        if kind in ("full", "full128"):
            _MODELS[kind] = RALENet("full", leads=2, L=model_L(kind), max_batch=16, train=False, device=DEV, seed=11).eval()
        else:
            _MODELS[kind] = NewRALE(RALENet("full", leads=2, L=400, max_batch=8, train=False, device=DEV, seed=11), seed=12).eval()
    return _MODELS[kind]


def _leads(kind):
    return 12 if kind == "newrale" else 2


def model_L(kind):
    return {"full": 64, "full128": 128, "newrale": 400}[kind]


def _signal(R, leads, T, seed):
    return torch.from_numpy(U.adc_records(R, leads, T, seed).astype(np.float32))


# ------------------------------------------------------------------------------------------------ 1. against the fixture
@pytest.mark.parametrize("fs_in,fs_out", U.PAIRS)
def test_convert_matches_scipy(fs_in, fs_out):
    """Every fixture case with leads 1, 2, 12 and R = 1, 3.  The fixture has two rows per case; row (r, lead) of a group is
    fixture row (r * leads + lead) % 2 times 2^-((r * leads + lead) // 2): a power of two scales every product and sum
    exactly, in fp32 as in fp64, so the expected row is scipy's times the same factor and no two rows of a group are equal.
    1e-5 rel-L2 and 1e-5 of max|x| per row: the project's forward tolerance (a strict-fp32 restatement of the sum on the
    CPU, `rate_util.convert(..., dtype=np.float32)`, deviates from fp64 by about 5e-7 of max|x| at most on such data)."""
    from ecg_denoise_amd import Resampler
    g = np.load(GOLDEN)
    rs = Resampler(fs_in, fs_out, DEV)
    assert (rs.up, rs.down) == U.ratio(fs_in, fs_out)
    worst = [0.0, 0.0]
    for T in U.LENGTHS[(fs_in, fs_out)]:
        x2, y2 = g[f"x_{fs_in}_{fs_out}_{T}"].astype(np.float64), g[f"y_{fs_in}_{fs_out}_{T}"]
        for leads in (1, 2, 12):
            for R in (1, 3):
                i = np.arange(R * leads)
                f = (2.0 ** -(i // 2))[:, None]
                x = (x2[i % 2] * f).reshape(R, leads, T)
                want = (y2[i % 2] * f).reshape(R, leads, -1)
                got = rs.convert(x.astype(np.float32) if R > 1 else torch.from_numpy(x[0].astype(np.float32)))
                assert got.is_cuda and got.dtype == torch.float32
                assert tuple(got.shape) == (want.shape if R > 1 else want.shape[1:])
                d = got.double().cpu().numpy().reshape(R * leads, -1) - want.reshape(R * leads, -1)
                xm = np.max(np.abs(x.reshape(R * leads, -1)), axis=1)
                l2 = np.sqrt((d ** 2).sum(1) / (want.reshape(R * leads, -1) ** 2).sum(1)).max()
                el = (np.abs(d).max(1) / xm).max()
                worst = [max(worst[0], l2), max(worst[1], el)]
                assert l2 <= 1e-5 and el <= 1e-5, (T, leads, R, l2, el)
    print(f"{fs_in}->{fs_out}: worst rel-L2 {worst[0]:.2e}, worst elementwise {worst[1]:.2e} of max|x|")


def test_convert_identity_and_refusals():
    from ecg_denoise_amd import RalError, Resampler
    x = _signal(2, 3, 50, 1).to(DEV)
    assert torch.equal(Resampler(360, 360, DEV).convert(x), x)
    assert torch.equal(Resampler(500, 500.0, DEV).convert(x[0]), x[0])
    with pytest.raises(RalError, match="not integral"):
        Resampler(499.5, 360, DEV)
    with pytest.raises(RalError, match="up=1 down=360"):
        Resampler(360, 1, DEV)
    with pytest.raises(RalError):
        Resampler(500, 360, DEV).convert(torch.zeros(5))
    with pytest.raises(RalError):
        Resampler(500, 360, DEV).convert(torch.zeros(2, 0))


# ------------------------------------------------------------------------------------------------ 2. pool equals record
def _drive(pool, recs, rng, chunk_sizes, omit=0.3, on_open=None):
    """feed the records through a pool, one stream each, opened at different calls, in random chunks; yields (stream, samples
    sent, closed, samples received so far) after every call that names the stream, then (stream, None, True, its whole output)"""
    n_streams = len(recs)
    sid, pos, outs, done = {}, {}, {i: [] for i in range(n_streams)}, set()
    call = 0
    while len(done) < n_streams:
        for i in range(n_streams):           # stream i opens at call 2 i, or when a slot has become free
            if i not in sid and call >= 2 * i and len(pool.open_streams) < pool.capacity:
                sid[i], pos[i] = pool.open(), 0
                if on_open:
                    on_open(sid[i])
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
            if i not in done and sid[i] in res:      # (a finished stream's sid may be another stream's by now)
                pos[i] += chunks[sid[i]].shape[1] if sid[i] in chunks else 0
                outs[i].append(res[sid[i]])
                yield i, pos[i], sid[i] in close, sum(o.shape[1] for o in outs[i])
                if sid[i] in close:
                    done.add(i)
    for i in range(n_streams):
        yield i, None, True, torch.cat(outs[i], dim=1)


@pytest.mark.parametrize("fs_in,fs_out,leads", [(500, 360, 12), (360, 500, 2), (257, 360, 1), (360, 128, 2)])
def test_pool_equals_record_bit_for_bit(fs_in, fs_out, leads):
    from ecg_denoise_amd import Resampler, ResamplerPool, rate_frontier, rate_length
    rng = np.random.default_rng(fs_in + fs_out + leads)
    lengths = [300, 3000, 1117, 2050, 641]
    recs = [_signal(1, leads, T, seed=T)[0].to(DEV) for T in lengths]
    rs = Resampler(fs_in, fs_out, DEV)
    pool = ResamplerPool(fs_in, fs_out, leads, capacity=3, device=DEV)     # five streams through three slots: slots are reused
    nan_slot = lambda sid: pool.hist[:, sid].fill_(float("nan"))           # a slot, fresh or reused: nothing before sample 0 may be read
    up, down = pool.up, pool.down
    tile = 1024
    for i, n, closed, got in _drive(pool, recs, rng, [1, 1, 2, 33, 700, 4 * tile * down // up + 13], on_open=nan_slot):
        if n is None:
            want = rs.convert(recs[i])
            assert got.shape == want.shape and torch.equal(got, want), (i, lengths[i])
        elif closed:
            assert got == rate_length(lengths[i], up, down)
        else:
            assert got == rate_frontier(n, up, down), (i, n)
    assert pool.open_streams == ()


def test_pool_one_sample_chunks_and_a_stream_alone():
    """1-sample chunks from the first sample to the last, and a stream alone against the same stream in a crowd"""
    from ecg_denoise_amd import Resampler, ResamplerPool
    recs = [_signal(1, 2, T, seed=T)[0].to(DEV) for T in (90, 61)]
    want = [Resampler(500, 360, DEV).convert(r) for r in recs]
    pool = ResamplerPool(500, 360, 2, capacity=2, device=DEV)
    a = pool.open()
    alone = [pool.push({a: recs[0][:, t:t + 1]}) for t in range(90)]
    alone = torch.cat([o[a] for o in alone] + [pool.close(a)], dim=1)
    assert torch.equal(alone, want[0])
    a, b = pool.open(), pool.open()
    outs = {a: [], b: []}
    for t in range(90):
        res = pool.push({s: r[:, t:t + 1] for s, r in ((a, recs[0]), (b, recs[1])) if t < r.shape[1]},
                        close=(b,) if t == 60 else ())
        for s, o in res.items():
            outs[s].append(o)
    outs[a].append(pool.close(a))
    assert torch.equal(torch.cat(outs[a], dim=1), want[0]) and torch.equal(torch.cat(outs[b], dim=1), want[1])


def test_pool_history_planes_hold_the_last_samples_received():
    """the history itself (tests/slot_util.py): chunks around hist_len = 28, a slot reused after both its planes were set to
    NaN; and the results of all four streams still equal the record path's bit for bit"""
    from slot_util import run_with_history_checks
    from ecg_denoise_amd import Resampler, ResamplerPool
    pool = ResamplerPool(500, 360, leads=2, capacity=3, device=DEV)
    assert pool.hist_len == 28
    recs = [_signal(1, 2, T, seed=T)[0].to(DEV) for T in (140, 85, 133, 70)]
    rs = Resampler(500, 360, DEV)
    for rec, outs in zip(recs, run_with_history_checks(pool, recs)):
        assert torch.equal(torch.cat(outs, dim=1), rs.convert(rec))


# ------------------------------------------------------------------------------------------------ 3. calls that raise
def test_pool_raising_calls_change_nothing():
    from ecg_denoise_amd import RalError, ResamplerPool, _lib
    from ecg_denoise_amd.model import _ptr, _stream
    pool = ResamplerPool(500, 360, 2, capacity=3, device=DEV)
    a, b = pool.open(), pool.open()
    x = _signal(1, 2, 400, 3)[0]
    pool.push({a: x[:, :100], b: x[:, :37]})
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
    with pytest.raises(RalError):
        pool.samples_in(2)
    # the entry point checks the host table before it launches anything: rows that would leave their buffers
    sids, tab = pool.plan({a: (2, 50), b: (2, 50)})
    xp = torch.zeros(100 * 2, device=DEV)
    out = torch.zeros(max(int(tab["m"].sum()), 1) * 2, device=DEV)
    tab_dev = torch.empty(len(tab) * tab.itemsize, dtype=torch.uint8, device=DEV)

    def call(t, x_total=100, out_total=None, hist_len=None, up=None):
        return _lib.lib().ral_rate_pool(_ptr(pool.hist), _ptr(xp), x_total, t.ctypes.data, len(t), _ptr(tab_dev), 1, pool.capacity,
                                        2, up or pool.up, pool.down, _ptr(pool.bank), pool.bank.numel(),
                                        pool.hist_len if hist_len is None else hist_len, _ptr(out),
                                        int(tab["m"].sum()) if out_total is None else out_total, _stream())

    def broken(field, row, value):
        t = tab.copy()
        t[field][row] = value
        return t

    for t, kw, rule in ((broken("slot", 1, 3), {}, "0 <= slot < capacity"),
                        (broken("slot", 1, int(tab["slot"][0])), {}, "every slot at most once"),
                        (broken("x_off", 1, 51), {}, "the chunk inside the packed chunks"),
                        (broken("out_off", 1, int(tab["out_off"][1]) + 1), {}, "the emitted samples inside the packed output"),
                        (broken("m", 1, int(tab["m"][1]) + 1), {"out_total": 10 ** 6}, "outputs that are final"),
                        (broken("n0", 1, int(tab["n0"][1]) + 1000), {}, "outputs that are final|inside the history"),
                        (broken("m0", 0, 0), {}, "inside the history"),
                        (broken("turn", 0, 2), {}, "turn 0 or 1"),
                        (broken("T", 0, 5), {}, "T = n0 \\+ c"),
                        (tab, {"hist_len": pool.hist_len - 1}, "hist_len >= 2 half / up \\+ 1"),
                        (tab, {"up": 36}, "lowest terms|ntaps")):
        assert call(t, **kw) != 0
        msg = _lib.lib().ral_last_error().decode()
        assert msg.startswith("rate_pool: need ") and __import__("re").search(rule, msg), msg
        unchanged()
    assert call(tab) == 0                      # the sound table runs
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 4. RateStreamingDenoiser
@pytest.mark.parametrize("kind", ["full", "newrale"])
@pytest.mark.parametrize("fs", [500, 250])
def test_rate_streaming_denoiser_is_the_explicit_composition(kind, fs):
    from ecg_denoise_amd import RalError, RateStreamingDenoiser, Resampler
    from ecg_denoise_amd.infer import StreamingDenoiser
    model, leads = _model(kind), _leads(kind)
    T = 1501 if fs == 500 else 977
    rec = _signal(2, leads, T, seed=fs + leads).to(DEV)
    for overlap in (0, 32):
        rsd = RateStreamingDenoiser(model, fs, overlap=overlap, use_graph=False)
        got = rsd.denoise(rec)
        assert got.shape == rec.shape and got.is_cuda
        sd = StreamingDenoiser(model, overlap=overlap, use_graph=False)
        mid = sd.denoise(Resampler(fs, 360, DEV).convert(rec))
        want = Resampler(360, fs, DEV).convert(mid)[..., :T]
        assert torch.equal(got, want)
        assert torch.equal(rsd.denoise(rec[0]), want[0])           # a single record
    short = (rsd.L * fs) // 360 - 2                                # converts to fewer than L samples
    with pytest.raises(RalError, match="shorter than one window"):
        rsd.denoise(rec[..., :short])
    with pytest.raises(RalError):
        rsd.denoise(rec[:, :1])


@pytest.mark.parametrize("kind", ["full", "newrale"])
def test_rate_streaming_denoiser_at_the_model_rate(kind):
    from ecg_denoise_amd import RateStreamingDenoiser
    from ecg_denoise_amd.infer import StreamingDenoiser
    model, leads = _model(kind), _leads(kind)
    rec = _signal(2, leads, 1000, seed=9).to(DEV)
    got = RateStreamingDenoiser(model, 360, overlap=32, use_graph=False).denoise(rec)
    assert torch.equal(got, StreamingDenoiser(model, overlap=32, use_graph=False).denoise(rec))


# ------------------------------------------------------------------------------------------------ 5. RateLivePool
@pytest.mark.parametrize("kind,overlap", [("full", 0), ("full", 32), ("full128", 64), ("newrale", 0), ("newrale", 64)])
def test_rate_live_pool_equals_rate_streaming_denoiser(kind, overlap):
    """(an overlap must stay below L: the L = 64 model takes 0 and 32, the same model with L = 128 takes 64)"""
    from ecg_denoise_amd import RalError, RateLivePool, RateStreamingDenoiser
    model, leads = _model(kind), _leads(kind)
    fs = 500 if overlap == 0 else 250
    rng = np.random.default_rng(overlap + leads)
    lengths = [1700, 900, 2300, 1203] if fs == 500 else [850, 450, 1150, 601]
    recs = [_signal(1, leads, T, seed=T + 1)[0].to(DEV) for T in lengths]
    rsd = RateStreamingDenoiser(model, fs, overlap=overlap, use_graph=False)
    want = [rsd.denoise(r) for r in recs]
    pool = RateLivePool(model, fs, capacity=3, overlap=overlap)
    for i, n, closed, got in _drive(pool, recs, rng, [1, 7, 90, 400, 1000]):
        if n is None:
            assert got.shape[1] == lengths[i] and torch.equal(got, want[i]), (i, lengths[i])
    assert pool.open_streams == () and pool.inner.open_streams == () and pool.back.open_streams == ()
    # a stream alone equals the same stream in the crowd above
    a = pool.open()
    parts = [pool.push({a: recs[1][:, t:t + 250]}) for t in range(0, lengths[1] - 250, 250)]
    t = (lengths[1] - 250 + 249) // 250 * 250
    alone = torch.cat([p[a] for p in parts] + [pool.close(a, recs[1][:, t:])], dim=1)
    assert torch.equal(alone, want[1])
    # a call that raises changes nothing: closing a stream that is shorter than one window at the model's rate
    a, b = pool.open(), pool.open()
    pool.push({a: recs[0][:, :300], b: recs[2][:, :40]})
    state = lambda: [p.hist.clone() for p in (pool.front, pool.inner, pool.back)] + \
        [s.n.copy() for s in (pool.front.state, pool.inner.state, pool.back.state)] + \
        [s.turn.copy() for s in (pool.front.state, pool.inner.state, pool.back.state)]
    before = state()
    with pytest.raises(RalError, match="shorter than one window"):
        pool.push({a: recs[0][:, 300:400]}, close=(b,))
    with pytest.raises(RalError, match="empty chunk"):
        pool.push({a: recs[0][:, 300:400], b: recs[2][:, 40:40]})
    with pytest.raises(RalError):
        pool.push({a: recs[0][:1, 300:400]})
    assert all(torch.equal(p, q) if torch.is_tensor(p) else np.array_equal(p, q) for p, q in zip(state(), before))
    assert pool.samples_in(a) == 300 and pool.samples_in(b) == 40
    rest = pool.push({a: recs[0][:, 300:]}, close=(a,))[a]
    assert rest.shape[1] <= lengths[0]


# ------------------------------------------------------------------------------------------------ 6. evaluate
def test_rate_evaluate_is_the_explicit_composition():
    from ecg_denoise_amd import RateStreamingDenoiser, mix_records, score_records
    model = _model("full")
    rec = _signal(3, 2, 1400, seed=4).to(DEV)
    noise = torch.randn(2, 5000, generator=torch.Generator().manual_seed(1)).to(DEV)
    rsd = RateStreamingDenoiser(model, 500, overlap=32, use_graph=False)
    got = rsd.evaluate(rec, noise, [0.0, 6.0, -3.0], offsets=[5, 700, 3000])
    noisy, clean = mix_records(rec, noise, [0.0, 6.0, -3.0], offsets=[5, 700, 3000])
    want = score_records(clean, rsd.denoise(noisy), noisy, window=rsd.window)
    assert rsd.window == -(-64 * 500 // 360) and got.window == want.window
    for k in ("per_lead", "per_record", "per_window", "window_mean"):
        assert torch.equal(getattr(got, k), getattr(want, k)), k
    assert torch.isfinite(got.window_mean).all()
