"""Live streams (LiveDenoiser; ral_live_windows / ral_live_emit): the kernels against the offline streaming kernels, the
concatenated live output against StreamingDenoiser on the complete records, graph against eager, stream independence,
reset, interleaved objects, weights that change after a capture, and the refused configurations."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L0 = 256


def _lib():
    from ecg_denoise_amd import _lib
    return _lib


def _p(t):
    from ecg_denoise_amd.model import _ptr
    return _ptr(t)


def _s():
    from ecg_denoise_amd.model import _stream
    return _stream()


def _records(S, leads, T, seed):
    """ECG-like records: a beat train with per-stream scale and offset, plus noise"""
    g = torch.Generator().manual_seed(seed)
    scale = 0.5 + torch.rand(S, leads, 1, generator=g)
    off = torch.randn(S, leads, 1, generator=g)
    t = torch.arange(T, dtype=torch.float32) / 360.0
    beat = torch.exp(-((t * (1.0 + 0.3 * torch.rand(S, 1, 1, generator=g))) % 1.0 - 0.3) ** 2 / 2e-4)
    return (beat * scale + off + 0.3 * torch.randn(S, leads, T, generator=g)).contiguous()


def _live(ld, rec, npush, final):
    """push npush chunks of rec, flush the rest (`final`: pass the remainder to flush, or None when there is none)"""
    C = ld.C
    outs = [ld.push(rec[:, :, i * C:(i + 1) * C]) for i in range(npush)]
    rest = rec[:, :, npush * C:]
    outs.append(ld.flush(rest if rest.shape[2] or final == "x" else None))
    return torch.cat(outs, dim=2)


_MODELS = {}


def _model(kind, leads=2, L=L0, max_batch=8):
    """one model per configuration for the module (the eval forward is the same whoever calls it)"""
    from ecg_denoise_amd import ACDAE, DANet, RALENet, UNet
    key = (kind, leads, L, max_batch)
    if key not in _MODELS:
        if kind in ("full", "nra"):
            m = RALENet(kind, leads=leads, L=L, max_batch=max_batch, train=False, device=DEV, seed=11)
        elif kind == "unet":
            m = UNet(leads=leads, L=L, max_batch=max_batch, train=False, device=DEV, seed=12)
        elif kind == "acdae":
            m = ACDAE(L=L, max_batch=max_batch, train=False, device=DEV, seed=13)
        else:
            m = DANet(L=L, max_batch=max_batch, train=False, device=DEV, seed=14)
        m.eval()
        _MODELS[key] = m
    return _MODELS[key]


# ---- the eval forward of a window does not depend on its batch --------------------------------------------------------
@pytest.mark.parametrize("kind,leads", [("full", 2), ("nra", 1), ("unet", 2), ("acdae", 2), ("danet", 2)])
def test_eval_forward_is_independent_of_batch_size_and_position(kind, leads):
    """the live path batches other windows together than the offline one: its outputs are bitwise equal to the offline ones
    only because a window's eval forward does not depend on the batch it runs in"""
    m = _model(kind, leads, max_batch=64)
    x = torch.randn(64, leads, L0, generator=torch.Generator().manual_seed(5)).to(DEV)
    ref = m(x).clone()
    for nb in (1, 3, 17, 64):
        perm = torch.randperm(64, generator=torch.Generator().manual_seed(nb)).to(DEV)
        xs = x[perm].contiguous()
        y = torch.cat([m(xs[i:i + nb].contiguous()) for i in range(0, 64, nb)])
        torch.cuda.synchronize()
        assert torch.equal(y, ref[perm]), (kind, nb)


# ---- kernel parity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [0, 34, 64])
def test_live_windows_equal_stream_windows_bitwise(overlap):
    S, leads, L = 3, 2, L0
    hop, C = L - overlap, 2 * (L - overlap)
    n0 = 5 * hop                                       # samples before the chunk
    T = n0 + C
    rec = _records(S, leads, T, 1).to(DEV)
    n_off = (T - L) // hop + 1 + (1 if (T - L) % hop else 0)
    win_off = torch.full((S * n_off, leads, L), float("nan"), device=DEV)
    st_off = torch.full((S * n_off * leads * 2,), float("nan"), device=DEV)
    _lib().check(_lib().lib().ral_stream_windows(_p(rec), S, T, leads, L, hop, 0, S * n_off, _p(win_off), _p(st_off), _s()))
    k0 = (n0 - L) // hop + 1
    nw = (T - L) // hop + 1 - k0
    hist = rec[:, :, n0 - L:n0].contiguous()
    x = rec[:, :, n0:].contiguous()
    hist_out = torch.full_like(hist, float("nan"))
    win = torch.full((S * nw, leads, L), float("nan"), device=DEV)
    st = torch.full((S * nw * leads * 2,), float("nan"), device=DEV)
    for w0, nb in ((0, 2), (2, S * nw - 2)):           # in two batches; the history written once
        _lib().check(_lib().lib().ral_live_windows(_p(hist), _p(x), _p(hist_out if w0 == 0 else None), S, leads, L, hop, C,
                                                   n0 - L, k0, nw, -1, w0, nb, _p(win[w0:]), _p(st), _s()))
    torch.cuda.synchronize()
    idx = torch.tensor([s * n_off + k0 + j for s in range(S) for j in range(nw)], device=DEV)
    assert torch.equal(win, win_off[idx])
    assert torch.equal(st.view(-1, leads, 2), st_off.view(-1, leads, 2)[idx])
    assert torch.equal(hist_out, rec[:, :, T - L:])


@pytest.mark.parametrize("overlap", [0, 34, 64])
@pytest.mark.parametrize("tail", [0, 7])
def test_live_emit_equals_stream_stitch_bitwise(overlap, tail):
    """the samples of the windows of a push (open stream) and of a flush (stream end known, right-aligned last window) equal
    the matching slices of the stitched record"""
    from ecg_denoise_amd.infer import live_frontier
    S, leads, L = 3, 2, L0
    hop = L - overlap
    T = 6 * hop + L + tail
    n_reg = (T - L) // hop + 1
    n_off = n_reg + (1 if (T - L) % hop else 0)
    g = torch.Generator().manual_seed(2)
    y = torch.randn(S * n_off, leads, L, generator=g).to(DEV)
    stats = torch.stack([torch.randn(S * n_off * leads, generator=g), 0.5 + torch.rand(S * n_off * leads, generator=g)], 1)
    stats = stats.reshape(-1).contiguous().to(DEV)
    out_off = torch.empty(S, leads, T, device=DEV)
    _lib().check(_lib().lib().ral_stream_stitch(_p(y), _p(stats), S, T, leads, L, hop, _p(out_off), _s()))

    def emit(k0, nw, Tk, lo, m, last=None):
        yy = y.view(S, n_off, leads, L)[:, k0:k0 + nw].reshape(-1, leads, L).contiguous()
        ss = stats.view(S, n_off, leads, 2)[:, k0:k0 + nw].reshape(-1).contiguous()
        out = torch.full((S, leads, m), float("nan"), device=DEV)
        ly, ls = (torch.full((S, leads, L), float("nan"), device=DEV), torch.full((S * leads * 2,), float("nan"), device=DEV)) \
            if last else (None, None)
        _lib().check(_lib().lib().ral_live_emit(_p(yy), _p(ss), S, leads, L, hop, k0, nw, Tk, 0, S * nw, lo, m, _p(out),
                                                _p(ly), _p(ls), _s()))
        return out, ly, ls

    # a push of 2 windows after the first 3 (open stream), keeping the last window
    n0, n1 = 2 * hop + L, 4 * hop + L
    lo, hi = live_frontier(n0, L, hop), live_frontier(n1, L, hop)
    out, ly, ls = emit(3, 2, -1, lo, hi - lo, last=True)
    torch.cuda.synchronize()
    assert torch.equal(out, out_off[:, :, lo:hi])
    assert torch.equal(ly, y.view(S, n_off, leads, L)[:, 4])
    assert torch.equal(ls.view(S, leads, 2), stats.view(S, n_off, leads, 2)[:, 4])
    # the first window of a stream keeps from sample 0
    out, _, _ = emit(0, 2, -1, 0, live_frontier(L + hop, L, hop))
    assert torch.equal(out, out_off[:, :, :live_frontier(L + hop, L, hop)])
    # the end of the stream: every window from k0 on, with T known
    k0 = n_reg - 2
    lo = live_frontier(k0 * hop + L - 1, L, hop) if k0 else 0
    out, _, _ = emit(k0, n_off - k0, T, lo, T - lo)
    torch.cuda.synchronize()
    assert torch.equal(out, out_off[:, :, lo:])


# ---- live against offline ---------------------------------------------------------------------------------------------
def _final_r(npush, C, L, hop, where):
    if where == "L":
        return None
    r = (L - npush * C) % hop                          # T on the hop grid
    return r if where == "grid" else r + 7


def _check_live(m, S, C, overlap, where, seed, use_graph=True):
    from ecg_denoise_amd.infer import LiveDenoiser, StreamingDenoiser
    L = m.eng.L
    hop = L - overlap
    if where == "L":                                   # a record of exactly one window
        npush, T = L // C, L
    else:
        npush = -(-2 * L // C) + 3
        T = npush * C + _final_r(npush, C, L, hop, where)
    rec = _records(S, m.eng.leads, T, seed)
    ref = StreamingDenoiser(m, overlap=overlap, use_graph=False).denoise(rec.to(DEV))
    got = _live(LiveDenoiser(m, streams=S, chunk=C, overlap=overlap, use_graph=use_graph), rec, npush, "x")
    torch.cuda.synchronize()
    assert got.shape == ref.shape
    assert torch.equal(got, ref), (got - ref).abs().max().item()
    return rec, got


@pytest.mark.parametrize("where", ["grid", "off", "L"])
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("cmul", [1, 3])
@pytest.mark.parametrize("overlap", [0, 64, 34])
@pytest.mark.parametrize("kind,leads", [("full", 2), ("nra", 1)])
def test_live_equals_offline(kind, leads, overlap, cmul, S, where):
    m = _model(kind, leads)
    _check_live(m, S, cmul * (L0 - overlap), overlap, where, seed=10 * overlap + cmul + S)


@pytest.mark.parametrize("kind", ["unet", "acdae", "danet"])
def test_live_equals_offline_baselines(kind):
    m = _model(kind)
    _check_live(m, 3, 2 * (L0 - 64), 64, "off", seed=3)
    _check_live(m, 2, L0, 0, "grid", seed=4)


def test_every_push_emits_C_samples_after_the_lag():
    from ecg_denoise_amd.infer import LiveDenoiser, live_frontier
    m = _model("full")
    overlap, S = 34, 2
    hop = L0 - overlap
    ld = LiveDenoiser(m, streams=S, chunk=hop, overlap=overlap)
    rec = _records(S, 2, 10 * hop, 5)
    n = 0
    for i in range(10):
        y = ld.push(rec[:, :, i * hop:(i + 1) * hop])
        n += hop
        assert y.shape == (S, 2, live_frontier(n, L0, hop) - live_frontier(n - hop, L0, hop))
        if n - hop >= L0:
            assert y.shape[2] == hop and ld.samples_in - (live_frontier(n, L0, hop)) == ld.latency
    assert ld.samples_in == 10 * hop


# ---- graph, isolation, lifecycle ----------------------------------------------------------------------------------------
def test_graph_replay_equals_eager_pushes():
    from ecg_denoise_amd.infer import LiveDenoiser
    m = _model("full")
    S, overlap = 5, 64
    C = 3 * (L0 - overlap)
    rec = _records(S, 2, 12 * C + 11, 6)
    a = _live(LiveDenoiser(m, S, C, overlap, use_graph=True), rec, 12, "x")
    b = _live(LiveDenoiser(m, S, C, overlap, use_graph=False), rec, 12, "x")
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_streams_are_independent():
    from ecg_denoise_amd.infer import LiveDenoiser
    m = _model("full")
    S, overlap = 5, 34
    C = L0 - overlap
    rec = _records(S, 2, 9 * C + 50, 7)
    perm = torch.tensor([3, 0, 4, 2, 1])
    a = _live(LiveDenoiser(m, S, C, overlap), rec, 9, "x")
    b = _live(LiveDenoiser(m, S, C, overlap), rec[perm].contiguous(), 9, "x")
    torch.cuda.synchronize()
    assert torch.equal(b, a[perm.to(DEV)])


def test_reset_then_reuse_equals_a_fresh_object():
    from ecg_denoise_amd.infer import LiveDenoiser
    m = _model("full")
    S, overlap = 3, 64
    C = L0 - overlap
    r1, r2 = _records(S, 2, 8 * C + 20, 8), _records(S, 2, 7 * C + 3, 9)
    ld = LiveDenoiser(m, S, C, overlap)
    for i in range(6):                                  # into the steady state (both graphs captured), then abandoned
        ld.push(r1[:, :, i * C:(i + 1) * C])
    ld.reset()
    assert ld.samples_in == 0
    a = _live(ld, r2, 7, "x")
    b = _live(LiveDenoiser(m, S, C, overlap), r2, 7, "x")
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    c = _live(ld, r1, 8, "x")                            # and again after a flush (which resets)
    d = _live(LiveDenoiser(m, S, C, overlap), r1, 8, "x")
    torch.cuda.synchronize()
    assert torch.equal(c, d)


def test_two_objects_on_one_model_interleaved():
    from ecg_denoise_amd.infer import LiveDenoiser, StreamingDenoiser
    m = _model("full")
    oa, ob = 0, 64
    Ca, Cb = L0, 2 * (L0 - ob)
    ra, rb = _records(2, 2, 10 * Ca, 10), _records(3, 2, 10 * Cb + 5, 11)
    la, lb = LiveDenoiser(m, 2, Ca, oa), LiveDenoiser(m, 3, Cb, ob)
    outa, outb = [], []
    for i in range(10):
        outa.append(la.push(ra[:, :, i * Ca:(i + 1) * Ca]))
        outb.append(lb.push(rb[:, :, i * Cb:(i + 1) * Cb]))
    outa.append(la.flush())
    outb.append(lb.flush(rb[:, :, 10 * Cb:]))
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(outa, 2), StreamingDenoiser(m, overlap=oa, use_graph=False).denoise(ra.to(DEV)))
    assert torch.equal(torch.cat(outb, 2), StreamingDenoiser(m, overlap=ob, use_graph=False).denoise(rb.to(DEV)))


# ---- weights that change after a capture ------------------------------------------------------------------------------
def _stale_case(change):
    """capture (both parities), change the weights, push on: the result equals a fresh eager object on the new weights"""
    from ecg_denoise_amd import RALENet
    from ecg_denoise_amd.infer import LiveDenoiser
    m = RALENet("full", leads=2, L=L0, max_batch=16, train=True, device=DEV, seed=21)
    m.eval()
    S, overlap = 3, 64
    C = L0 - overlap
    rec = _records(S, 2, 14 * C + 9, 12)
    ld = LiveDenoiser(m, S, C, overlap, use_graph=True)
    outs = [ld.push(rec[:, :, i * C:(i + 1) * C]) for i in range(6)]
    assert all(g is not None for g in ld.graphs)
    change(m)
    ld2 = LiveDenoiser(m, S, C, overlap, use_graph=False)
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
    return m


def test_stale_graph_after_load_state_dict():
    from ecg_denoise_amd import RALENet
    other = RALENet("full", leads=2, L=L0, max_batch=16, train=False, device=DEV, seed=99)

    def change(m):
        before = m(torch.ones(1, 2, L0, device=DEV)).clone()
        m.load_state_dict(other.state_dict())
        assert not torch.equal(m(torch.ones(1, 2, L0, device=DEV)), before)
    _stale_case(change)


def test_stale_graph_after_train_steps():
    def change(m):
        m.train()
        g = torch.Generator().manual_seed(3)
        for _ in range(2):
            x = torch.randn(16, 2, L0, generator=g).to(DEV)
            m.train_step(x + 0.1 * torch.randn(16, 2, L0, generator=g).to(DEV), x)
        m.eval()
    _stale_case(change)


# ---- refused configurations -----------------------------------------------------------------------------------------------
def test_refused_configurations():
    from ecg_denoise_amd import NewRALE
    from ecg_denoise_amd.infer import LiveDenoiser
    RalError = _lib().RalError
    m = _model("full")
    nr = NewRALE(m, seed=1)
    with pytest.raises(RalError, match="NewRALE"):
        LiveDenoiser(nr, streams=2, chunk=L0)
    for chunk in (0, -L0, L0 - 64 + 1, (L0 - 64) // 2):
        with pytest.raises(RalError, match="chunk"):
            LiveDenoiser(m, streams=2, chunk=chunk, overlap=64)
    for overlap in (-2, 3, L0, L0 + 2):
        with pytest.raises(RalError, match="overlap"):
            LiveDenoiser(m, streams=2, chunk=L0, overlap=overlap)
    ld = LiveDenoiser(m, streams=2, chunk=64, overlap=L0 - 64)
    ld.push(torch.randn(2, 2, 64))
    with pytest.raises(RalError, match="shorter than one window"):
        ld.flush(torch.randn(2, 2, L0 - 129))
    with pytest.raises(RalError):
        ld.push(torch.randn(2, 2, 65))


# ---- a realistic run ----------------------------------------------------------------------------------------------------------
def test_long_run_matches_offline():
    """64 streams x 10 minutes at 360 Hz in 1-second chunks (L = 512, overlap 152: hop = C = 360)"""
    from ecg_denoise_amd import RALENet
    from ecg_denoise_amd.infer import LiveDenoiser, StreamingDenoiser
    m = RALENet("full", leads=2, L=512, max_batch=1024, train=False, device=DEV, seed=31)
    m.eval()
    S, C, overlap, secs = 64, 360, 152, 600
    rec = _records(S, 2, secs * C, 13).to(DEV)
    ld = LiveDenoiser(m, streams=S, chunk=C, overlap=overlap)
    outs = [ld.push(rec[:, :, i * C:(i + 1) * C]) for i in range(secs)]
    outs.append(ld.flush())
    got = torch.cat(outs, 2)
    ref = StreamingDenoiser(m, batch=1024, overlap=overlap).denoise(rec)
    torch.cuda.synchronize()
    assert torch.equal(got, ref), (got - ref).abs().max().item()
