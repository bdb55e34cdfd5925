"""The stream pool (LivePool; ral_pool_windows / ral_pool_emit): the kernels against the offline streaming kernels with streams
at different positions in one launch, a seeded schedule of independent streams against StreamingDenoiser on the complete
records, tenancy, lockstep against LiveDenoiser, calls that raise in the middle of a schedule, and weights that change between
two calls.  Every comparison is bitwise.  tests/test_gpu_newrale_pool.py runs the same cases through the 12-lead adapter."""
import numpy as np
import pytest
import torch

from test_gpu_live import DEV, L0, _lib, _model, _p, _records, _s

pytestmark = pytest.mark.gpu
CHUNKS = lambda L, hop: (1, 7, 360, hop, L + 3, 3 * L + 5)


class Generic:
    """the 1- and 2-lead entry points behind one calling convention (Adapter in test_gpu_newrale_pool.py is the 12-lead one)"""
    inner = leads = 2

    def windows_off(self, rec, T, L, hop, n):
        win = torch.full((n, self.leads, L), float("nan"), device=DEV)
        st = torch.full((n * self.leads * 2,), float("nan"), device=DEV)
        _lib().check(_lib().lib().ral_stream_windows(_p(rec), 1, T, self.leads, L, hop, 0, n, _p(win), _p(st), _s()))
        return win, st

    def stitch_off(self, y, st, T, L, hop, n):
        out = torch.full((self.leads, T), float("nan"), device=DEV)
        _lib().check(_lib().lib().ral_stream_stitch(_p(y), _p(st), 1, T, self.leads, L, hop, _p(out), _s()))
        return out

    def windows_pool(self, hist, xp, x_total, tab, tab_dev, upload, cap, L, hop, write_hist, w0, nb, win, st):
        return _lib().lib().ral_pool_windows(_p(hist), _p(xp), x_total, tab.ctypes.data, len(tab), _p(tab_dev), upload, cap,
                                             self.leads, L, hop, write_hist, w0, nb, _p(win), _p(st), _s())

    def emit_pool(self, y, st, tab, tab_dev, upload, cap, L, hop, w0, nb, from_last, out, out_total, ly, ls):
        return _lib().lib().ral_pool_emit(_p(y), _p(st), tab.ctypes.data, len(tab), _p(tab_dev), upload, cap, self.leads, L, hop,
                                          w0, nb, from_last, _p(out), out_total, _p(ly), _p(ls), _s())


def _n_windows(T, L, hop):
    return (T - L) // hop + 1 + (1 if (T - L) % hop else 0)


def _rows(L, hop, streams):
    """streams: (slot, n0, c, closing, turn) -> the table the host planner gives for them"""
    from ecg_denoise_amd.infer import pool_plan
    tab = np.zeros(len(streams), dtype=_lib().POOL_ROW)
    for r, (slot, n0, c, closing, turn) in enumerate(streams):
        k0, nw, lo, m, T = (int(v) for v in pool_plan(n0, c, closing, L, hop))
        tab[r] = (n0, T, k0, lo, 0, 0, 0, slot, c, nw, m, turn, 0 if closing else _lib().POOL_KEEP)
    for col, src in (("x_off", "c"), ("out_off", "m"), ("w_off", "nw")):
        tab[col] = np.cumsum(tab[src]) - tab[src]
    return tab


def _positions(L, hop):
    """five streams at different positions in one launch: mid-stream on the hop grid, before its first window, ending off the
    grid after a long chunk, and two short chunks that complete no window (history only), one of them a stream's first"""
    return [(2, 5 * hop + L, 2 * hop, False, 1), (0, 100, L + 3, False, 0), (3, L + 7, 2 * hop + 11, True, 1),
            (5, 0, 5, False, 0), (1, L + 1, 5, False, 1)]


def check_pool_windows_equal_stream_windows(api, L, overlap):
    hop, cap, leads = L - overlap, 6, api.leads
    streams = _positions(L, hop)
    tab = _rows(L, hop, streams)
    recs = [_records(1, leads, n0 + c, 40 + r).to(DEV) for r, (_, n0, c, _, _) in enumerate(streams)]
    hist = torch.full((2, cap, leads, L), float("nan"), device=DEV)     # NaN wherever nothing may be read
    xs = []
    for rec, (slot, n0, c, _, turn) in zip(recs, streams):
        have = min(n0, L)
        hist[turn, slot, :, L - have:] = rec[0, :, n0 - have:n0]
        xs.append(rec[0, :, n0:].reshape(-1))
    xp = torch.cat(xs)
    total, x_total = int(tab["nw"].sum()), int(tab["c"].sum())
    win = torch.full((total, api.inner, L), float("nan"), device=DEV)
    st = torch.full((total * leads * 2,), float("nan"), device=DEV)
    tab_dev = torch.empty(tab.nbytes, dtype=torch.uint8, device=DEV)
    before = hist.clone()
    for w0, nb in ((0, 2), (2, total - 2)):            # in two batches; the table uploaded and the histories written once
        _lib().check(api.windows_pool(hist, xp, x_total, tab, tab_dev, int(w0 == 0), cap, L, hop, int(w0 == 0), w0, nb,
                                      win[w0:], st))
    torch.cuda.synchronize()
    written = torch.zeros(2, cap, dtype=torch.bool)
    for rec, row, (slot, n0, c, closing, turn) in zip(recs, tab, streams):
        T = n0 + c
        k, w = int(row["k0"]), int(row["w_off"])
        if row["nw"]:
            # (a window of an open stream is a regular one: the same samples as window k + j of the record cut at n0 + c)
            win_off, st_off = api.windows_off(rec, T, L, hop, _n_windows(T, L, hop))
            torch.cuda.synchronize()
        for j in range(int(row["nw"])):
            assert torch.equal(win[w + j], win_off[k + j]), (slot, j)
            assert torch.equal(st.view(-1, leads, 2)[w + j], st_off.view(-1, leads, 2)[k + j]), (slot, j)
        if not closing:
            want = torch.zeros(leads, L, device=DEV)
            have = min(T, L)
            want[:, L - have:] = rec[0, :, T - have:]
            assert torch.equal(hist[1 - turn, slot], want), slot
            written[1 - turn, slot] = True
    same = ~written.to(DEV)
    assert torch.equal(torch.nan_to_num(hist[same], nan=7.0), torch.nan_to_num(before[same], nan=7.0))   # nothing else written
    assert not torch.isnan(win).any() and not torch.isnan(st).any()


def check_pool_emit_equals_stream_stitch(api, L, overlap):
    hop, cap, leads = L - overlap, 6, api.leads
    streams = _positions(L, hop)
    if overlap:               # a stream on the hop grid that ends without a chunk: its kept last window gives [lo, T)
        streams.append((4, 3 * hop + L, 0, True, 0))
    tab = _rows(L, hop, streams)
    total, out_total = int(tab["nw"].sum()), int(tab["m"].sum())
    g = torch.Generator().manual_seed(2)
    y = torch.randn(max(total, 1), api.inner, L, generator=g).to(DEV)
    st = torch.stack([torch.randn(total * leads, generator=g), 0.5 + torch.rand(total * leads, generator=g)], 1).reshape(-1).to(DEV)
    last_y = torch.full((cap, api.inner, L), float("nan"), device=DEV)
    last_st = torch.full((cap, leads, 2), float("nan"), device=DEV)
    out = torch.full((out_total * leads,), float("nan"), device=DEV)
    tab_dev = torch.empty(tab.nbytes, dtype=torch.uint8, device=DEV)
    for w0, nb in ((0, 3), (3, total - 3)):
        _lib().check(api.emit_pool(y[w0:], st, tab, tab_dev, int(w0 == 0), cap, L, hop, w0, nb, 0, out, out_total, last_y, last_st))
    if overlap:
        # the kept window of slot 4: as if an earlier call had kept it
        ky = torch.randn(api.inner, L, generator=g).to(DEV)
        ks = torch.stack([torch.randn(leads, generator=g), 0.5 + torch.rand(leads, generator=g)], 1).to(DEV)
        last_y[4], last_st[4] = ky, ks
        last = tab[-1:].copy()
        last["k0"] -= 1
        last["nw"], last["w_off"] = 1, 0
        last_dev = torch.empty(last.nbytes, dtype=torch.uint8, device=DEV)
        _lib().check(api.emit_pool(last_y, last_st, last, last_dev, 1, cap, L, hop, 0, 1, 1, out, out_total, None, None))
    torch.cuda.synchronize()
    for row, (slot, n0, c, closing, turn) in zip(tab, streams):
        # the offline record that has this call's windows at their numbers: the stream's end if known, else the end of the
        # call's last window (every window up to there is regular in both)
        k0, nw, lo, m, w = (int(row[f]) for f in ("k0", "nw", "lo", "m", "w_off"))
        got = out[int(row["out_off"]) * leads:(int(row["out_off"]) + m) * leads].view(leads, m)
        if nw == 0 and not (closing and overlap):
            assert m == 0
            continue
        T = n0 + c if closing else (k0 + nw - 1) * hop + L
        n = _n_windows(T, L, hop)
        yy = torch.randn(n, api.inner, L, generator=g).to(DEV)
        ss = torch.stack([torch.randn(n * leads, generator=g), 0.5 + torch.rand(n * leads, generator=g)], 1).to(DEV)
        yy[k0:k0 + nw], ss.view(n, leads, 2)[k0:k0 + nw] = y[w:w + nw], st.view(-1, leads, 2)[w:w + nw]
        if nw == 0:
            yy[k0 - 1], ss.view(n, leads, 2)[k0 - 1] = ky, ks
        ref = api.stitch_off(yy, ss.reshape(-1).contiguous(), T, L, hop, n)
        torch.cuda.synchronize()
        assert torch.equal(got, ref[:, lo:lo + m]), slot
        if not closing:
            assert torch.equal(last_y[slot], y[w + nw - 1]) and torch.equal(last_st[slot], st.view(-1, leads, 2)[w + nw - 1])
    kept = [s[0] for s, row in zip(streams, tab) if not s[3] and row["nw"]] + ([4] if overlap else [])
    rest = torch.tensor([s not in kept for s in range(cap)], device=DEV)
    assert torch.isnan(last_y[rest]).all() and torch.isnan(last_st[rest]).all()
    assert not torch.isnan(out).any()


@pytest.mark.parametrize("overlap", [0, 34, 64])
def test_pool_windows_equal_stream_windows_bitwise(overlap):
    check_pool_windows_equal_stream_windows(Generic(), L0, overlap)


@pytest.mark.parametrize("overlap", [0, 34, 64])
def test_pool_emit_equals_stream_stitch_bitwise(overlap):
    check_pool_emit_equals_stream_stitch(Generic(), L0, overlap)


def test_the_table_of_the_refusal_tests_runs():
    """tests/test_pool_cpu.py refuses edits of one table; that table itself is accepted by both entry points"""
    from test_pool_cpu import GOOD, _good_rows
    tab, a, api = _good_rows(), GOOD, Generic()
    hist = torch.randn(2, a["capacity"], 2, a["L"], device=DEV)
    xp = torch.randn(a["x_total"] * 2, device=DEV)
    win = torch.full((3, 2, a["L"]), float("nan"), device=DEV)
    st = torch.full((3 * 2 * 2,), float("nan"), device=DEV)
    out = torch.full((a["out_total"] * 2,), float("nan"), device=DEV)
    tab_dev = torch.empty(tab.nbytes, dtype=torch.uint8, device=DEV)
    ly, ls = torch.zeros(a["capacity"], 2, a["L"], device=DEV), torch.zeros(a["capacity"], 2, 2, device=DEV)
    _lib().check(api.windows_pool(hist, xp, a["x_total"], tab, tab_dev, 1, a["capacity"], a["L"], a["hop"], 1, 0, 3, win, st))
    _lib().check(api.emit_pool(win, st, tab, tab_dev, 0, a["capacity"], a["L"], a["hop"], 0, 3, 0, out, a["out_total"], ly, ls))
    torch.cuda.synchronize()
    assert not torch.isnan(win).any() and not torch.isnan(out).any()
    assert torch.equal(ly[0], win[0])


# ---- a schedule of independent streams ----------------------------------------------------------------------------------
def make_schedule(L, hop, leads, seed, n_streams=13, capacity=5, batch_cap=8):
    """-> (records, calls): calls is a list of (opens, {stream: (a, b)}, closes), streams by index.  Lengths on and off the hop
    grid and one of exactly L; stream 0 arrives in one chunk of many more windows than `batch_cap`; different start calls;
    chunk lengths from CHUNKS; calls that name only some of the open streams; streams closed with their last chunk or in a later
    call without one; at most `capacity` open at a time, so slots are reused - by streams of very different amplitude."""
    rng = np.random.default_rng(seed)
    lens = [5 * batch_cap * hop + L + 3, L, L + 3 * hop, 2 * L + hop + 7] + \
           [int(rng.integers(L, 6 * L)) for _ in range(n_streams - 4)]
    recs = [(_records(1, leads, T, seed * 100 + i)[0] * float(10.0 ** ((i * 5) % 7 - 3))).contiguous() for i, T in enumerate(lens)]
    start = [0, 0, 1, 0] + [int(rng.integers(0, 12)) for _ in range(n_streams - 4)]
    with_chunk = [True, True, False] + [bool(rng.integers(0, 2)) for _ in range(n_streams - 3)]
    pos, state = [0] * n_streams, ["wait"] * n_streams            # wait -> open -> (drained ->) done
    calls, t = [], 0
    while any(s != "done" for s in state):
        opens, chunks, closes = [], {}, []
        for i in range(n_streams):
            if state[i] == "wait" and start[i] <= t and sum(s in ("open", "drained") for s in state) < capacity:
                state[i] = "open"
                opens.append(i)
        for i in range(n_streams):
            if state[i] == "drained" and rng.random() < 0.6:
                closes.append(i)
                state[i] = "done"
            elif state[i] == "open" and (rng.random() < 0.7 or i in opens):
                c = lens[i] if i == 0 else int(rng.choice(CHUNKS(L, hop)))
                a, b = pos[i], min(pos[i] + c, lens[i])
                chunks[i], pos[i] = (a, b), b
                if b == lens[i]:
                    if with_chunk[i]:
                        closes.append(i)
                        state[i] = "done"
                    else:
                        state[i] = "drained"
        if opens or chunks or closes:
            calls.append((opens, chunks, closes))
        t += 1
    return recs, calls


def run_schedule(pool, recs, calls, device_chunks=False, between=None):
    """-> per stream, the list of tensors the pool returned for it, in order"""
    sid, pieces = {}, {i: [] for i in range(len(recs))}
    for ci, (opens, chunks, closes) in enumerate(calls):
        for i in opens:
            sid[i] = pool.open()
        if between is not None:
            between(ci, pool, sid)
        if not chunks and not closes:
            continue
        x = {sid[i]: (recs[i][:, a:b].to(DEV) if device_chunks and i % 2 else recs[i][:, a:b]) for i, (a, b) in chunks.items()}
        got = pool.push(x, close=[sid[i] for i in closes])
        assert sorted(got) == sorted({sid[i] for i in list(chunks) + closes})
        for i in set(list(chunks) + closes):
            pieces[i].append(got[sid[i]])
            assert pool.state.is_open[sid[i]] == (i not in closes)
            if i not in closes:
                assert pool.samples_in(sid[i]) == chunks[i][1]
    assert pool.open_streams == ()
    return pieces


def check_against_offline(m, pieces, recs, overlap, batch=None):
    from ecg_denoise_amd.infer import StreamingDenoiser, live_frontier
    sd = StreamingDenoiser(m, overlap=overlap, use_graph=False, **({"batch": batch} if batch else {}))
    for i, rec in enumerate(recs):
        ref = sd.denoise(rec.to(DEV))
        got = torch.cat(pieces[i], dim=1)
        torch.cuda.synchronize()
        assert got.shape == ref.shape, i
        assert torch.equal(got, ref), (i, (got - ref).abs().max().item())


def check_frontier(pieces, calls, L, hop):
    """after every call a stream that has received n samples has been given exactly [0, live_frontier(n))"""
    from ecg_denoise_amd.infer import live_frontier
    given, idx = {}, {}
    for opens, chunks, closes in calls:
        for i in set(list(chunks) + closes):
            j = idx.get(i, 0)
            given[i] = given.get(i, 0) + pieces[i][j].shape[1]
            idx[i] = j + 1
            if i not in closes:
                assert given[i] == live_frontier(chunks[i][1], L, hop), i


@pytest.mark.parametrize("kind,leads,overlap", [("full", 2, 34), ("full", 2, 0), ("nra", 1, 64), ("unet", 2, 34), ("acdae", 2, 64),
                                                ("danet", 2, 0)])
def test_pool_equals_offline(kind, leads, overlap):
    from ecg_denoise_amd import LivePool
    m = _model(kind, leads)
    hop = L0 - overlap
    recs, calls = make_schedule(L0, hop, leads, seed=3 + overlap)
    assert max(sum(-(-(b - a) // hop) for a, b in ch.values()) for _, ch, _ in calls) >= 5 * 8      # several batches in one call
    pool = LivePool(m, capacity=5, overlap=overlap)
    assert (pool.capacity, pool.L, pool.hop, pool.leads) == (5, L0, hop, leads)
    pieces = run_schedule(pool, recs, calls, device_chunks=True)
    check_frontier(pieces, calls, L0, hop)
    check_against_offline(m, pieces, recs, overlap)


def check_tenancy(make_pool, recs, calls, who):
    """stream `who` alone in a pool of one slot, cut as in the crowd: the same tensors, call by call"""
    crowd = run_schedule(make_pool(5), recs, calls)
    alone_calls = [([0] if who in o else [], {0: ch[who]} if who in ch else {}, [0] if who in cl else [])
                   for o, ch, cl in calls if who in o or who in ch or who in cl]
    alone = run_schedule(make_pool(1), [recs[who]], alone_calls)
    torch.cuda.synchronize()
    assert len(alone[0]) == len(crowd[who]) > 1
    for a, b in zip(alone[0], crowd[who]):
        assert torch.equal(a, b)


def test_a_stream_alone_equals_the_stream_in_the_crowd():
    from ecg_denoise_amd import LivePool
    m = _model("full")
    recs, calls = make_schedule(L0, L0 - 34, 2, seed=37)
    for who in (3, 7):
        check_tenancy(lambda cap: LivePool(m, capacity=cap, overlap=34), recs, calls, who)


def check_lockstep(m, make_live, make_pool, leads, L, overlap, S=5):
    hop = L - overlap
    C = 2 * hop
    rec = _records(S, leads, 7 * C + 11, 6)
    ld, pool = make_live(S, C), make_pool(S)
    sids = [pool.open() for _ in range(S)]
    for i in range(7):
        a = ld.push(rec[:, :, i * C:(i + 1) * C])
        b = pool.push({sid: rec[s, :, i * C:(i + 1) * C] for s, sid in enumerate(sids)})
        torch.cuda.synchronize()
        assert torch.equal(a, torch.stack([b[sid] for sid in sids])), i
    a = ld.flush(rec[:, :, 7 * C:])
    b = pool.push({sid: rec[s, :, 7 * C:] for s, sid in enumerate(sids)}, close=sids)
    torch.cuda.synchronize()
    assert torch.equal(a, torch.stack([b[sid] for sid in sids]))


@pytest.mark.parametrize("overlap", [0, 64])
def test_pool_in_lockstep_equals_live_denoiser(overlap):
    from ecg_denoise_amd import LiveDenoiser, LivePool
    m = _model("full")
    check_lockstep(m, lambda S, C: LiveDenoiser(m, S, C, overlap), lambda S: LivePool(m, S, overlap), 2, L0, overlap)


def check_raising_calls(m, pool, recs, calls, overlap, leads, L):
    """every Python-side refusal in the middle of the schedule, alone and beside valid chunks of other streams: nothing
    changes, the schedule finishes and matches offline.  The pool has one slot more than the schedule uses; it holds a short
    stream that cannot be closed yet."""
    RalError = _lib().RalError
    extra = _records(1, leads, L + 5, 77)[0]
    tmp = pool.open()
    assert pool.push({tmp: extra[:, :3]})[tmp].shape == (leads, 0)
    seen = []

    def between(ci, pool, sid):
        if ci != len(calls) // 2:
            return
        live = [s for s in pool.open_streams if s != tmp]
        assert live
        ok = {live[0]: torch.randn(leads, 9)}
        free = [s for s in range(pool.capacity) if s not in pool.open_streams]
        state = (pool.state.n.copy(), pool.state.turn.copy(), pool.state.is_open.copy(), list(pool.state.free))
        hist, ly = pool.hist.clone(), pool.last_y.clone()
        bad = [dict(chunks={99: torch.randn(leads, 9)}), dict(chunks={**ok, -1: torch.randn(leads, 9)}),
               dict(chunks={**ok, tmp: torch.randn(leads + 1, 9)}), dict(chunks={**ok, tmp: torch.randn(leads, 0)}),
               dict(chunks={tmp: torch.randn(9)}), dict(chunks=ok, close=[tmp]), dict(chunks={**ok, tmp: torch.randn(leads, 9)}, close=[tmp]),
               dict(chunks={}, close=[]), dict(chunks=ok, close=[99])]
        if free:
            bad.append(dict(chunks={**ok, free[0]: torch.randn(leads, 9)}))       # a closed (or never opened) sid
        for kw in bad:
            with pytest.raises(RalError):
                pool.push(**kw)
            seen.append(kw)
        with pytest.raises(RalError):
            pool.close(tmp)
        with pytest.raises(RalError):
            pool.samples_in(99)
        torch.cuda.synchronize()
        after = (pool.state.n, pool.state.turn, pool.state.is_open, pool.state.free)
        assert all(np.array_equal(x, y) for x, y in zip(state, after))
        assert torch.equal(hist, pool.hist) and torch.equal(ly, pool.last_y)

    pieces = _run_with_guest(pool, recs, calls, between, tmp)
    assert len(seen) >= 9
    rest = [pool.push({tmp: extra[:, 3:L]})[tmp], pool.close(tmp, extra[:, L:])]
    check_against_offline(m, {**pieces, len(recs): rest}, recs + [extra], overlap)


def _run_with_guest(pool, recs, calls, between, guest):
    """run_schedule with one more stream open throughout (its final check expects an empty pool)"""
    sid, pieces = {}, {i: [] for i in range(len(recs))}
    for ci, (opens, chunks, closes) in enumerate(calls):
        for i in opens:
            sid[i] = pool.open()
        between(ci, pool, sid)
        if not chunks and not closes:
            continue
        got = pool.push({sid[i]: recs[i][:, a:b] for i, (a, b) in chunks.items()}, close=[sid[i] for i in closes])
        for i in set(list(chunks) + closes):
            pieces[i].append(got[sid[i]])
    assert pool.open_streams == (guest,)
    return pieces


def test_a_call_that_raises_changes_nothing():
    from ecg_denoise_amd import LivePool
    m = _model("full")
    recs, calls = make_schedule(L0, L0 - 64, 2, seed=5, n_streams=8)
    check_raising_calls(m, LivePool(m, capacity=6, overlap=64), recs, calls, 64, 2, L0)


def test_weights_changed_between_two_calls_are_used():
    from ecg_denoise_amd import LivePool, RALENet
    mk = lambda seed, train: RALENet("full", leads=2, L=L0, max_batch=16, train=train, device=DEV, seed=seed).eval()
    m, old, other = mk(21, True), mk(21, False), mk(99, False)
    overlap, S = 64, 3
    rec = _records(S, 2, 9 * 360 + 5, 12)
    pools = [LivePool(m, S, overlap), LivePool(old, S, overlap)]
    sids = [[p.open() for _ in range(S)] for p in pools]
    feed = lambda p, ids, i, close=(): p.push({sid: rec[s, :, i * 360:(i + 1) * 360] for s, sid in enumerate(ids)}, close=close)
    for i in range(4):
        a, b = feed(pools[0], sids[0], i), feed(pools[1], sids[1], i)
        torch.cuda.synchronize()
        assert all(torch.equal(a[x], b[y]) for x, y in zip(*sids))            # the same weights so far
    m.load_state_dict(other.state_dict())
    fresh = LivePool(m, S, overlap)                                            # the new weights from the start
    fids = [fresh.open() for _ in range(S)]
    for i in range(4):
        feed(fresh, fids, i)
    for i in range(4, 9):
        a, b, c = feed(pools[0], sids[0], i), feed(pools[1], sids[1], i), feed(fresh, fids, i)
        torch.cuda.synchronize()
        # (a call emits from the windows it runs itself, so the very next call is all new weights)
        assert all(torch.equal(a[x], c[y]) for x, y in zip(sids[0], fids)), i
        assert any(not torch.equal(a[x], b[y]) for x, y in zip(*sids)), i


def test_refused_models_and_geometry():
    from ecg_denoise_amd import LivePool, NewRALE
    RalError = _lib().RalError
    m = _model("full")
    with pytest.raises(RalError, match="NewRALELivePool"):
        LivePool(NewRALE(m, seed=1), 4)
    for overlap in (-2, 3, L0, L0 + 2):
        with pytest.raises(RalError, match="overlap"):
            LivePool(m, 4, overlap=overlap)
    pool = LivePool(m, 2)
    a, b = pool.open(), pool.open()
    with pytest.raises(RalError, match="slots"):
        pool.open()
    assert pool.open_streams == (a, b)
    out = pool.close(a, torch.randn(2, L0))
    assert out.shape == (2, L0) and pool.open() == a
