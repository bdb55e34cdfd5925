"""Live 12-lead streams through `NewRALE` (NewRALELiveDenoiser; ral_newrale_live_front / ral_newrale_live_back): the batch
independence that exact comparison rests on, the live kernels against the record kernel and against the unfused launches,
the concatenated live output against StreamingDenoiser on the complete records, graph against eager, lag, stream
independence, reset, weights that change after a capture, and the refused configurations."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib():
    from ecg_denoise_amd import _lib
    return _lib


def _p(t):
    from ecg_denoise_amd.model import _ptr
    return _ptr(t)


def _s():
    from ecg_denoise_amd.model import _stream
    return _stream()


def _n_windows(T, L, hop):
    return (T - L) // hop + 1 + (1 if (T - L) % hop else 0)


def _records(S, T, seed):
    """12-lead ECG-like records: a beat train with per-stream and per-lead scale and offset, plus noise"""
    g = torch.Generator().manual_seed(seed)
    scale = 0.5 + torch.rand(S, 12, 1, generator=g)
    off = torch.randn(S, 12, 1, generator=g)
    t = torch.arange(T, dtype=torch.float32) / 360.0
    beat = torch.exp(-((t * (1.0 + 0.3 * torch.rand(S, 1, 1, generator=g))) % 1.0 - 0.3) ** 2 / 2e-4)
    return (beat * scale + off + 0.3 * torch.randn(S, 12, T, generator=g)).contiguous()


def _adapter_params(seed):
    """a flat adapter buffer in NewRALE's layout (every tensor padded to 4 floats) -> (device tensor, offsets)"""
    from ecg_denoise_amd import NewRALE
    off, cur = {}, 0
    for k, shp in NewRALE.SHAPES.items():
        off[k] = cur
        cur += (int(np.prod(shp)) + 3) // 4 * 4
    g = torch.Generator().manual_seed(seed)
    prm = torch.zeros(cur)
    for k, shp in NewRALE.SHAPES.items():
        n = int(np.prod(shp))
        prm[off[k]:off[k] + n] = (torch.rand(n, generator=g) * 2 - 1) / math.sqrt(12 * 13)
    return prm.to(DEV), off


def _conv(prm, off, name, x, cout, lrelu):
    y = torch.empty(x.shape[0], cout, x.shape[2], device=DEV)
    _lib().check(_lib().lib().ral_conv13_forward(_p(x), _p(prm[off[name + ".weight"]:]), _p(prm[off[name + ".bias"]:]), _p(y),
                                                 x.shape[0], x.shape[1], cout, x.shape[2], int(lrelu), _s()))
    return y


_MODELS = {}


def _model(L, max_batch=8, seed=11):
    """one eval-mode NewRALE per configuration for the module (its eval forward is the same whoever calls it)"""
    from ecg_denoise_amd import NewRALE, RALENet
    key = (L, max_batch, seed)
    if key not in _MODELS:
        inner = RALENet("full", leads=2, L=L, max_batch=max_batch, train=False, device=DEV, seed=seed)
        _MODELS[key] = NewRALE(inner, seed=seed + 1).eval()
    return _MODELS[key]


def _live(ld, rec, npush, final):
    """push npush chunks of rec, flush the rest (`final` "x": pass the remainder to flush even when it is empty; None: pass
    nothing when there is no remainder)"""
    C = ld.C
    outs = [ld.push(rec[:, :, i * C:(i + 1) * C]) for i in range(npush)]
    rest = rec[:, :, npush * C:]
    outs.append(ld.flush(rest if rest.shape[2] or final == "x" else None))
    return torch.cat(outs, dim=2)


# ---- 1. the eval forward of a window does not depend on its batch -------------------------------------------------------
@pytest.mark.parametrize("L", [1024, 400])
def test_eval_forward_is_independent_of_batch_size_and_position(L):
    """the live path batches other windows together than the offline one: its outputs are bitwise equal to the offline ones
    only because a window's eval forward does not depend on the batch it runs in"""
    m = _model(L, max_batch=64)
    x = torch.randn(64, 12, L, generator=torch.Generator().manual_seed(5)).to(DEV)
    ref = m(x).clone()
    for nb in (1, 3, 17, 64):
        perm = torch.randperm(64, generator=torch.Generator().manual_seed(nb)).to(DEV)
        xs = x[perm].contiguous()
        y = torch.cat([m(xs[i:i + nb].contiguous()).clone() for i in range(0, 64, nb)])
        torch.cuda.synchronize()
        assert torch.equal(y, ref[perm]), (L, nb)


# ---- 2. live front against the record kernel ----------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [0, 128, 6])
@pytest.mark.parametrize("closed", [False, True])
def test_live_front_equals_record_front_bitwise(overlap, closed):
    S, L = 3, 1024
    hop = L - overlap
    n0 = 4 * hop + L                                   # samples before the chunk
    C = 2 * hop + (37 if closed else 0)                # a closed stream ends off the grid: a right-aligned last window
    T = n0 + C
    rec = _records(S, T, 1 + overlap).to(DEV)
    prm, _ = _adapter_params(3)
    n_off = _n_windows(T, L, hop)
    in_off = torch.full((S * n_off, 2, L), float("nan"), device=DEV)
    st_off = torch.full((S * n_off * 24,), float("nan"), device=DEV)
    _lib().check(_lib().lib().ral_newrale_stream_front(_p(rec), S, T, L, hop, 0, S * n_off, _p(prm), _p(in_off), _p(st_off),
                                                       _s()))
    k0 = (n0 - L) // hop + 1
    nw = (n_off if closed else (T - L) // hop + 1) - k0
    hist = rec[:, :, n0 - L:n0].contiguous()
    x = rec[:, :, n0:].contiguous()
    hist_out = torch.full_like(hist, float("nan"))
    inner = torch.full((S * nw, 2, L), float("nan"), device=DEV)
    st = torch.full((S * nw * 24,), float("nan"), device=DEV)
    for w0, nb in ((0, 2), (2, S * nw - 2)):           # in two batches; the history written once
        _lib().check(_lib().lib().ral_newrale_live_front(_p(hist), _p(x), _p(hist_out if w0 == 0 else None), S, L, hop, C,
                                                         n0 - L, k0, nw, T if closed else -1, w0, nb, _p(prm), _p(inner[w0:]),
                                                         _p(st), _s()))
    torch.cuda.synchronize()
    idx = torch.tensor([s * n_off + k0 + j for s in range(S) for j in range(nw)], device=DEV)
    assert torch.equal(inner, in_off[idx])
    assert torch.equal(st.view(-1, 12, 2), st_off.view(-1, 12, 2)[idx])
    assert torch.equal(hist_out, rec[:, :, T - L:])
    # the history alone (nb = 0)
    h2 = torch.full_like(hist, float("nan"))
    _lib().check(_lib().lib().ral_newrale_live_front(_p(hist), _p(x), _p(h2), S, L, hop, C, n0 - L, k0, nw, T if closed else -1,
                                                     0, 0, _p(prm), _p(inner), _p(st), _s()))
    torch.cuda.synchronize()
    assert torch.equal(h2, rec[:, :, T - L:])


# ---- 3. live back against the unfused launches ----------------------------------------------------------------------------
@pytest.mark.parametrize("L,overlap", [(1024, 0), (1024, 128), (320, 6)])
def test_live_back_equals_unfused_emit_bitwise(L, overlap):
    """conv3 -> conv4 (ral_conv13_forward) -> ral_live_emit(leads = 12) with the same geometry, clipping of lo / m included,
    and the last window's inner output and statistics"""
    from ecg_denoise_amd.infer import live_frontier
    S = 3
    hop = L - overlap
    T = 6 * hop + L + 7
    n_reg = (T - L) // hop + 1
    n_off = _n_windows(T, L, hop)
    prm, off = _adapter_params(4)
    g = torch.Generator().manual_seed(2)
    iy = torch.randn(S * n_off, 2, L, generator=g).to(DEV)
    stats = torch.stack([torch.randn(S * n_off * 12, generator=g), 0.5 + torch.rand(S * n_off * 12, generator=g)], 1)
    stats = stats.reshape(-1).contiguous().to(DEV)
    y12 = _conv(prm, off, "conv4", _conv(prm, off, "conv3", iy, 6, True), 12, False)

    def run(fused, k0, nw, Tk, lo, m, last, batches):
        src = iy if fused else y12
        ch = 2 if fused else 12
        yy = src.view(S, n_off, ch, L)[:, k0:k0 + nw].reshape(-1, ch, L).contiguous()
        ss = stats.view(S, n_off, 12, 2)[:, k0:k0 + nw].reshape(-1).contiguous()
        out = torch.full((S, 12, m), float("nan"), device=DEV)
        ly = torch.full((S, ch, L), float("nan"), device=DEV) if last else None
        ls = torch.full((S * 24,), float("nan"), device=DEV) if last else None
        for w0, nb in batches:
            if fused:
                rc = _lib().lib().ral_newrale_live_back(_p(yy[w0:]), _p(ss), _p(prm), S, L, hop, k0, nw, Tk, w0, nb, lo, m,
                                                        _p(out), _p(ly), _p(ls), _s())
            else:
                rc = _lib().lib().ral_live_emit(_p(yy[w0:]), _p(ss), S, 12, L, hop, k0, nw, Tk, w0, nb, lo, m, _p(out), _p(ly),
                                                _p(ls), _s())
            _lib().check(rc)
        return out, ly, ls

    n0, n1 = 2 * hop + L, 4 * hop + L
    lo, hi = live_frontier(n0, L, hop), live_frontier(n1, L, hop)
    k0e = n_reg - 2
    lo_e = live_frontier(k0e * hop + L - 1, L, hop) if k0e else 0
    cases = [
        (3, 2, -1, lo, hi - lo, True, [(0, 2 * S)]),                   # a push of 2 windows, keeping the last one
        (3, 2, -1, lo, hi - lo, True, [(0, 4), (4, 2 * S - 4)]),       # the same in two batches
        (3, 2, -1, lo + 5, hi - lo - 20, True, [(0, 2 * S)]),          # clipped at both ends
        (0, 2, -1, 0, live_frontier(L + hop, L, hop), False, [(0, 2 * S)]),   # the first windows keep from sample 0
        (k0e, n_off - k0e, T, lo_e, T - lo_e, False, [(0, S * (n_off - k0e))]),   # the end of a closed stream
        (n_reg - 1, 1, T, lo_e + hop, T - lo_e - hop, False, [(0, S)]),   # flush: the last regular window alone
    ]
    for k0, nw, Tk, lo_, m, last, batches in cases:
        a, aly, als = run(True, k0, nw, Tk, lo_, m, last, batches)
        b, bly, bls = run(False, k0, nw, Tk, lo_, m, last, batches)
        torch.cuda.synchronize()
        assert torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num()), (k0, nw, Tk, lo_, m)
        if last:
            assert torch.equal(aly, iy.view(S, n_off, 2, L)[:, k0 + nw - 1])
            assert torch.equal(als, bls)


# ---- 4. live against offline ----------------------------------------------------------------------------------------------
def _check_live(m, S, C, overlap, T, npush, final, use_graph=True, seed=0):
    from ecg_denoise_amd.infer import NewRALELiveDenoiser, StreamingDenoiser
    rec = _records(S, T, seed)
    ref = StreamingDenoiser(m, overlap=overlap, use_graph=False).denoise(rec.to(DEV))
    got = _live(NewRALELiveDenoiser(m, streams=S, chunk=C, overlap=overlap, use_graph=use_graph), rec, npush, final)
    torch.cuda.synchronize()
    assert got.shape == ref.shape
    assert torch.equal(got, ref), (got - ref).abs().max().item()
    return rec, got


@pytest.mark.parametrize("where", ["grid", "off", "L", "long"])
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("cmul", [1, 3])
@pytest.mark.parametrize("overlap", [0, 128, 6])
@pytest.mark.parametrize("L", [1024, 400])
def test_live_equals_offline(L, overlap, cmul, S, where):
    """max_batch 8: at S = 5 and C = 3 hop a push spans two batches.  where: T on the hop grid (flushed with an empty last
    chunk), off it, exactly one window (flushed with nothing), or a last chunk that holds more windows than a push"""
    m = _model(L)
    hop = L - overlap
    C = cmul * hop
    if where == "L":
        npush, T, final = L // C, L, None
    else:
        npush = -(-2 * L // C) + 2
        r = (L - npush * C) % hop
        T = npush * C + {"grid": r, "off": r + 7, "long": r + 2 * C + 7}[where]
        final = "x"
    _check_live(m, S, C, overlap, T, npush, final, seed=10 * overlap + cmul + S)


# ---- 5. graph, lag, isolation, lifecycle ----------------------------------------------------------------------------------
def test_graph_replay_equals_eager_pushes():
    from ecg_denoise_amd.infer import NewRALELiveDenoiser
    m = _model(1024)
    S, overlap = 5, 128
    C = 3 * (1024 - overlap)
    rec = _records(S, 8 * C + 11, 6)
    a = _live(NewRALELiveDenoiser(m, S, C, overlap, use_graph=True), rec, 8, "x")
    b = _live(NewRALELiveDenoiser(m, S, C, overlap, use_graph=False), rec, 8, "x")
    torch.cuda.synchronize()
    assert torch.equal(a, b)


@pytest.mark.parametrize("L,overlap", [(1024, 128), (400, 6)])
def test_every_push_emits_C_samples_after_the_lag(L, overlap):
    from ecg_denoise_amd.infer import NewRALELiveDenoiser, live_frontier, live_latency
    m = _model(L)
    S = 2
    hop = L - overlap
    ld = NewRALELiveDenoiser(m, streams=S, chunk=hop, overlap=overlap)
    assert ld.latency == live_latency(L, hop)
    rec = _records(S, 8 * hop, 5)
    n = 0
    for i in range(8):
        y = ld.push(rec[:, :, i * hop:(i + 1) * hop])
        n += hop
        assert y.shape == (S, 12, live_frontier(n, L, hop) - live_frontier(n - hop, L, hop))
        if n - hop >= L:
            assert y.shape[2] == hop and ld.samples_in - live_frontier(n, L, hop) == ld.latency
    assert ld.samples_in == 8 * hop


def test_streams_are_independent():
    from ecg_denoise_amd.infer import NewRALELiveDenoiser
    m = _model(400)
    S, overlap = 5, 6
    C = 400 - overlap
    rec = _records(S, 9 * C + 50, 7)
    perm = torch.tensor([3, 0, 4, 2, 1])
    a = _live(NewRALELiveDenoiser(m, S, C, overlap), rec, 9, "x")
    b = _live(NewRALELiveDenoiser(m, S, C, overlap), rec[perm].contiguous(), 9, "x")
    torch.cuda.synchronize()
    assert torch.equal(b, a[perm.to(DEV)])


def test_reset_then_reuse_equals_a_fresh_object():
    from ecg_denoise_amd.infer import NewRALELiveDenoiser
    m = _model(400)
    S, overlap = 3, 128
    C = 400 - overlap
    r1, r2 = _records(S, 8 * C + 20, 8), _records(S, 7 * C + 3, 9)
    ld = NewRALELiveDenoiser(m, S, C, overlap)
    for i in range(6):                                  # into the steady state (both graphs captured), then abandoned
        ld.push(r1[:, :, i * C:(i + 1) * C])
    assert all(g is not None for g in ld.graphs)
    ld.reset()
    assert ld.samples_in == 0
    a = _live(ld, r2, 7, "x")
    b = _live(NewRALELiveDenoiser(m, S, C, overlap), r2, 7, "x")
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    c = _live(ld, r1, 8, "x")                            # and again after a flush (which resets)
    d = _live(NewRALELiveDenoiser(m, S, C, overlap), r1, 8, "x")
    torch.cuda.synchronize()
    assert torch.equal(c, d)


# ---- 6. weights that change after a capture ------------------------------------------------------------------------------
L_STALE = 256


def _stale_case(change):
    """capture (both parities), change the weights, push on: the result equals a fresh eager object on the new weights"""
    from ecg_denoise_amd import NewRALE, RALENet
    from ecg_denoise_amd.infer import NewRALELiveDenoiser
    m = NewRALE(RALENet("full", leads=2, L=L_STALE, max_batch=16, train=True, device=DEV, seed=21), seed=22).eval()
    S, overlap = 3, 64
    C = L_STALE - overlap
    rec = _records(S, 14 * C + 9, 12)
    ld = NewRALELiveDenoiser(m, S, C, overlap, use_graph=True)
    outs = [ld.push(rec[:, :, i * C:(i + 1) * C]) for i in range(6)]
    assert all(g is not None for g in ld.graphs)
    probe = torch.randn(2, 12, L_STALE, generator=torch.Generator().manual_seed(1)).to(DEV)
    before = m(probe).clone()
    change(m)
    assert not m.training
    assert not torch.equal(m(probe), before)
    ld2 = NewRALELiveDenoiser(m, S, C, overlap, use_graph=False)
    for i in range(6):
        ld2.push(rec[:, :, i * C:(i + 1) * C])           # the new weights' history (what the first 6 pushes emitted differs)
    for i in range(6, 14):
        outs.append(ld.push(rec[:, :, i * C:(i + 1) * C]))
        ref = ld2.push(rec[:, :, i * C:(i + 1) * C])
        torch.cuda.synchronize()
        assert torch.equal(outs[-1], ref), i
    a, b = ld.flush(rec[:, :, 14 * C:]), ld2.flush(rec[:, :, 14 * C:])
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def _other(seed):
    from ecg_denoise_amd import NewRALE, RALENet
    return NewRALE(RALENet("full", leads=2, L=L_STALE, max_batch=16, train=False, device=DEV, seed=seed), seed=seed + 1)


def test_stale_graph_after_adapter_load_state_dict():
    other = _other(99).state_dict()
    adapter_only = {k: v for k, v in other.items() if not k.startswith("rale.")}
    _stale_case(lambda m: m.load_state_dict(adapter_only))


def test_stale_graph_after_inner_load_state_dict():
    """the adapter's own generation does not move: only the (adapter, inner) pair tells the graphs are stale"""
    other = _other(98)

    def change(m):
        g = m.generation()
        m.rale.load_state_dict(other.rale.state_dict())
        assert m.generation()[0] == g[0] and m.generation()[1] != g[1]
    _stale_case(change)


def test_stale_graph_after_train_step():
    def change(m):
        m.train()
        g = torch.Generator().manual_seed(3)
        x = torch.randn(16, 12, L_STALE, generator=g).to(DEV)
        m.train_step(x + 0.1 * torch.randn(16, 12, L_STALE, generator=g).to(DEV), x)
        m.eval()
    _stale_case(change)


# ---- 7. refused configurations ----------------------------------------------------------------------------------------------
def test_refused_configurations():
    from ecg_denoise_amd import NewRALE, RALENet
    from ecg_denoise_amd.infer import NewRALELiveDenoiser
    RalError = _lib().RalError
    L = 256
    inner = RALENet("full", leads=2, L=L, max_batch=8, train=True, device=DEV, seed=41)
    m = NewRALE(inner, seed=42)
    with pytest.raises(RalError, match="NewRALE"):
        NewRALELiveDenoiser(inner, streams=2, chunk=L)
    for chunk in (0, -L, L - 64 + 1, (L - 64) // 2):
        with pytest.raises(RalError, match="chunk"):
            NewRALELiveDenoiser(m, streams=2, chunk=chunk, overlap=64)
    for overlap in (-2, 3, L, L + 2):
        with pytest.raises(RalError, match="overlap"):
            NewRALELiveDenoiser(m, streams=2, chunk=L, overlap=overlap)
    ld = NewRALELiveDenoiser(m, streams=2, chunk=64, overlap=L - 64)
    assert not m.training                              # the constructor puts the model in eval mode
    with pytest.raises(RalError, match="shape"):
        ld.push(torch.randn(2, 2, 64))                 # a 2-lead chunk
    with pytest.raises(RalError):
        ld.push(torch.randn(2, 12, 65))
    ld.push(torch.randn(2, 12, 64))
    with pytest.raises(RalError, match="shorter than one window"):
        ld.flush(torch.randn(2, 12, L - 129))
    m.train()
    with pytest.raises(RalError, match="eval"):
        ld.push(torch.randn(2, 12, 64))
    with pytest.raises(RalError, match="eval"):
        ld.flush(torch.randn(2, 12, L))
    m.eval()


# ---- 8. a realistic run -------------------------------------------------------------------------------------------------------
def test_long_run_matches_offline():
    """16 streams x 10 minutes at 360 Hz in 1-second chunks (L = 1024, overlap 664: hop = C = 360)"""
    from ecg_denoise_amd.infer import NewRALELiveDenoiser, StreamingDenoiser
    m = _model(1024, max_batch=1024, seed=31)
    S, C, overlap, secs = 16, 360, 664, 600
    rec = _records(S, secs * C, 13).to(DEV)
    ld = NewRALELiveDenoiser(m, streams=S, chunk=C, overlap=overlap)
    outs = [ld.push(rec[:, :, i * C:(i + 1) * C]) for i in range(secs)]
    outs.append(ld.flush())
    got = torch.cat(outs, 2)
    ref = StreamingDenoiser(m, batch=1024, overlap=overlap).denoise(rec)
    torch.cuda.synchronize()
    assert torch.equal(got, ref), (got - ref).abs().max().item()
