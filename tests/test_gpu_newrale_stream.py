"""12-lead records streamed through `NewRALE` (fused adapter kernels ral_newrale_stream_front / _back around the inner
RA-LENet), and `GraphedForward(NewRALE)`: against the unfused composition of the existing entry points, against the
fp64 oracle, graph against eager, and captured plans after the weights change."""
import math
from collections import OrderedDict

import numpy as np
import pytest
import torch

import ralenet_oracle as O
from parity_util import rel

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


def _records(R, T, seed):
    g = torch.Generator().manual_seed(seed)
    scale = 0.5 + torch.rand(R, 12, 1, generator=g)
    off = torch.randn(R, 12, 1, generator=g)
    t = torch.arange(T, dtype=torch.float32) / 360.0
    beat = torch.exp(-((t * 1.2) % 1.0 - 0.3) ** 2 / 2e-4)
    return (beat * scale + off + 0.5 * torch.randn(R, 12, T, generator=g)).contiguous()


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
        b = 1.0 / math.sqrt(12 * 13)
        prm[off[k]:off[k] + n] = (torch.rand(n, generator=g) * 2 - 1) * b
    return prm.to(DEV), off


def _conv(prm, off, name, x, cout, lrelu):
    y = torch.empty(x.shape[0], cout, x.shape[2], device=DEV)
    w = prm[off[name + ".weight"]:]
    b = prm[off[name + ".bias"]:]
    _lib().check(_lib().lib().ral_conv13_forward(_p(x), _p(w), _p(b), _p(y), x.shape[0], x.shape[1], cout, x.shape[2],
                                                 int(lrelu), _s()))
    return y


def _front(rec, L, hop, w0, nw, prm, n_all):
    R, _, T = rec.shape
    inner = torch.full((nw, 2, L), float("nan"), device=DEV)
    stats = torch.full((n_all * 24,), float("nan"), device=DEV)
    _lib().check(_lib().lib().ral_newrale_stream_front(_p(rec), R, T, L, hop, w0, nw, _p(prm), _p(inner), _p(stats), _s()))
    return inner, stats


def _unfused(m, rec, L, hop, batch):
    """the record pipeline from the existing entry points: ral_stream_windows(12) -> conv1 -> conv2 -> ral_forward ->
    conv3 -> conv4 -> ral_stream_stitch(12)"""
    lib = _lib().lib()
    R, _, T = rec.shape
    nw_all = R * _n_windows(T, L, hop)
    stats = torch.empty(nw_all * 24, device=DEV)
    y = torch.empty(nw_all, 12, L, device=DEV)
    win = torch.empty(min(batch, nw_all), 12, L, device=DEV)
    r = torch.empty(min(batch, nw_all), 2, L, device=DEV)
    for w0 in range(0, nw_all, batch):
        nw = min(batch, nw_all - w0)
        _lib().check(lib.ral_stream_windows(_p(rec), R, T, 12, L, hop, w0, nw, _p(win), _p(stats), _s()))
        a2 = _conv(m.params, m.off, "conv2", _conv(m.params, m.off, "conv1", win[:nw], 6, True), 2, True)
        _lib().check(lib.ral_forward(m.rale.eng.h, _p(a2), _p(r), nw, 0, _s()))
        y[w0:w0 + nw] = _conv(m.params, m.off, "conv4", _conv(m.params, m.off, "conv3", r[:nw], 6, True), 12, False)
    out = torch.empty(R, 12, T, device=DEV)
    _lib().check(lib.ral_stream_stitch(_p(y), _p(stats), R, T, 12, L, hop, _p(out), _s()))
    return out


def _model(L, max_batch, seed, train=False):
    from ecg_denoise_amd import NewRALE, RALENet
    m = NewRALE(RALENet("full", leads=2, L=L, max_batch=max_batch, train=train, device=DEV, seed=seed), seed=seed + 1)
    return m.eval()


# ---------------------------------------------------------------------------------------------------------------------
# 1. front kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,ov", [(1024, 0), (1024, 128), (320, 64)])
def test_front_matches_stream_windows_and_two_convs(L, ov):
    hop = L - ov
    R, T = 2, 4 * L + 37                              # right-aligned last window
    n = _n_windows(T, L, hop)
    assert (T - L) % hop
    rec = _records(R, T, L).to(DEV)
    prm, off = _adapter_params(5)
    for w0, nw in ((0, R * n), (n - 2, 3)):           # all windows; the end of record 0 and the start of record 1
        inner, stats = _front(rec, L, hop, w0, nw, prm, R * n)
        win = torch.empty(nw, 12, L, device=DEV)
        st = torch.full((R * n * 24,), float("nan"), device=DEV)
        _lib().check(_lib().lib().ral_stream_windows(_p(rec), R, T, 12, L, hop, w0, nw, _p(win), _p(st), _s()))
        ref = _conv(prm, off, "conv2", _conv(prm, off, "conv1", win, 6, True), 2, True)
        torch.cuda.synchronize()
        assert rel(inner.cpu().numpy(), ref.cpu().numpy()) <= 1e-6
        sl = slice(w0 * 24, (w0 + nw) * 24)
        assert rel(stats[sl].cpu().numpy(), st[sl].cpu().numpy()) <= 1e-6
        assert torch.isnan(stats[:w0 * 24]).all() and torch.isnan(stats[(w0 + nw) * 24:]).all()


def test_front_off_grid_length():
    """L = 400: a multiple of 16 only (ral_stream_windows takes multiples of 64): against a torch z-score + the convs"""
    L, ov = 400, 48
    hop = L - ov
    R, T = 2, 3 * L + 91
    starts = [k * hop for k in range((T - L) // hop + 1)] + ([T - L] if (T - L) % hop else [])
    n = len(starts)
    rec = _records(R, T, 9).to(DEV)
    prm, off = _adapter_params(6)
    inner, stats = _front(rec, L, hop, 0, R * n, prm, R * n)
    w = torch.stack([rec[r, :, s:s + L] for r in range(R) for s in starts])
    mu = w.mean(-1, keepdim=True)
    sd = w.std(-1, unbiased=False, keepdim=True).clamp_min(1e-6)
    ref = _conv(prm, off, "conv2", _conv(prm, off, "conv1", ((w - mu) / sd).contiguous(), 6, True), 2, True)
    torch.cuda.synchronize()
    assert rel(inner.cpu().numpy(), ref.cpu().numpy()) <= 1e-6
    assert rel(stats.cpu().numpy(), torch.cat([mu, sd], -1).cpu().numpy()) <= 1e-6     # (mean, std) pairs


# ---------------------------------------------------------------------------------------------------------------------
# 2. / 3. whole records at L = 1024, eager against the unfused composition, graph against eager
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def m1024():
    return _model(1024, 64, 11)


@pytest.mark.parametrize("ov", [0, 128])
def test_whole_record_eager_matches_unfused(m1024, ov):
    from ecg_denoise_amd.infer import StreamingDenoiser
    L, T = 1024, 30001
    rec = _records(2, T, 3).to(DEV)
    sd = StreamingDenoiser(m1024, batch=32, overlap=ov, use_graph=False)
    assert sd.leads == 12 and sd.L == L and 2 * sd.windows_per_record(T) > 32    # more than one batch
    out = sd.denoise(rec)
    ref = _unfused(m1024, rec, L, L - ov, 32)
    torch.cuda.synchronize()
    assert out.shape == rec.shape and torch.isfinite(out).all()
    assert rel(out.cpu().numpy(), ref.cpu().numpy()) <= 1e-6


@pytest.mark.parametrize("ov", [0, 128])
def test_whole_record_graph_equals_eager(m1024, ov):
    from ecg_denoise_amd.infer import StreamingDenoiser
    rec = _records(2, 30001, 4).to(DEV)
    eager = StreamingDenoiser(m1024, batch=32, overlap=ov, use_graph=False).denoise(rec)
    sd = StreamingDenoiser(m1024, batch=32, overlap=ov, use_graph=True)
    for _ in range(3):
        out = sd.denoise(rec)
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    single = sd.denoise(rec[1], copy=False)           # (12, T) input; a view of the plan's buffer
    assert single.shape == (12, 30001)


# ---------------------------------------------------------------------------------------------------------------------
# 4. against the fp64 oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_short_record_matches_fp64_oracle():
    from ecg_denoise_amd import NewRALE, RALENet
    from ecg_denoise_amd.infer import StreamingDenoiser
    L = 256
    T = 2 * L + 200
    p32 = O.init_params(O.ralenet_param_shapes("full", 2), 1234)
    pa32 = O.init_params(O.newrale_param_shapes(), 77)
    inner = RALENet("full", leads=2, L=L, max_batch=8, train=False, device=DEV)
    inner.load_state_dict(p32, strict=False)
    m = NewRALE(inner)
    m.load_state_dict(pa32)
    m.eval()
    rec = _records(1, T, 21)
    out = StreamingDenoiser(m, batch=8, overlap=0, use_graph=True).denoise(rec.to(DEV)).cpu().double()
    starts = [0, L, T - L]
    w = torch.stack([rec[0, :, s:s + L] for s in starts]).double()
    mu = w.mean(-1, keepdim=True)
    sdv = w.std(-1, unbiased=False, keepdim=True).clamp_min(1e-6)
    p = OrderedDict((k, v.double()) for k, v in p32.items())
    pa = OrderedDict((k, v.double()) for k, v in pa32.items())
    with torch.no_grad():
        y = O.newrale_forward(pa, p, (w - mu) / sdv, "full", False, None) * sdv + mu
    want = torch.cat([y[0], y[1], y[2][:, 2 * L - (T - L):]], dim=1)[None]     # the last window keeps what is left
    assert want.shape == out.shape
    assert rel(out.numpy(), want.numpy()) <= 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# 5. GraphedForward(NewRALE)
# ---------------------------------------------------------------------------------------------------------------------
def test_graphed_forward_newrale_equals_eval_call():
    from ecg_denoise_amd.infer import GraphedForward
    m = _model(256, 32, 3)
    x = torch.randn(32, 12, 256, device=DEV)
    ref = m(x).clone()
    g = GraphedForward(m, 32)
    for _ in range(3):
        y = g(x)
    torch.cuda.synchronize()
    assert y.shape == (32, 12, 256)
    assert torch.equal(y, ref)


# ---------------------------------------------------------------------------------------------------------------------
# 6. weights changed after a capture
# ---------------------------------------------------------------------------------------------------------------------
def test_weights_changed_after_capture_load_state_dict():
    from ecg_denoise_amd.infer import GraphedForward, StreamingDenoiser
    L, ov = 256, 64
    m = _model(L, 16, 30)
    other = _model(L, 16, 40).state_dict()         # other adapter AND inner weights
    rec = _records(2, 5001, 7).to(DEV)
    x = torch.randn(16, 12, L, device=DEV)
    sd = StreamingDenoiser(m, batch=16, overlap=ov, use_graph=True)
    g = GraphedForward(m, 16)
    out0 = sd.denoise(rec)
    y0 = g(x).clone()
    m.load_state_dict(other)                        # (the model stays in eval mode: no eval() that would mark the change too)
    assert not m.training
    out1 = sd.denoise(rec)
    y1 = g(x).clone()
    eager = StreamingDenoiser(m, batch=16, overlap=ov, use_graph=False).denoise(rec)
    ref = m(x)
    torch.cuda.synchronize()
    assert not torch.equal(out0, out1) and not torch.equal(y0, y1)
    assert torch.equal(out1, eager)
    assert torch.equal(y1, ref)


def test_weights_changed_after_capture_training_step():
    """a training step rewrites the adapter (read by pointer) and the inner model's BatchNorm running statistics (read by
    pointer); the inner weights stay frozen.  After it, and eval(), the captured plans give what a fresh eager run gives."""
    from ecg_denoise_amd.infer import GraphedForward, StreamingDenoiser
    L, ov = 256, 64
    m = _model(L, 16, 50, train=True)
    rec = _records(2, 5001, 8).to(DEV)
    x = torch.randn(16, 12, L, device=DEV)
    tgt = torch.randn(16, 12, L, device=DEV)
    sd = StreamingDenoiser(m, batch=16, overlap=ov, use_graph=True)
    g = GraphedForward(m, 16)
    out0 = sd.denoise(rec)
    y0 = g(x).clone()
    m.train()
    m.train_step(x, tgt)
    m.eval()
    out1 = sd.denoise(rec)
    y1 = g(x).clone()
    eager = StreamingDenoiser(m, batch=16, overlap=ov, use_graph=False).denoise(rec)
    ref = m(x)
    torch.cuda.synchronize()
    assert not torch.equal(out0, out1) and not torch.equal(y0, y1)
    assert torch.equal(out1, eager)
    assert torch.equal(y1, ref)


# ---------------------------------------------------------------------------------------------------------------------
# 7. input checks
# ---------------------------------------------------------------------------------------------------------------------
def test_input_checks():
    from ecg_denoise_amd.infer import StreamingDenoiser
    RalError = _lib().RalError
    m = _model(256, 16, 60)
    sd = StreamingDenoiser(m, batch=16, overlap=0, use_graph=False)
    with pytest.raises(RalError):
        sd.denoise(torch.randn(2, 11, 5000))       # wrong number of leads
    with pytest.raises(RalError):
        sd.denoise(torch.randn(2, 5000))           # a 2-lead record
    with pytest.raises(RalError):
        sd.denoise(torch.randn(12, 200))           # shorter than one window
    with pytest.raises(RalError):
        StreamingDenoiser(m, overlap=3)            # odd overlap


# ---------------------------------------------------------------------------------------------------------------------
# parameter generation: what moves it, and captures that leave each other's plans valid
# ---------------------------------------------------------------------------------------------------------------------
def test_generation_moves_on_weight_changes_only():
    m = _model(256, 16, 70, train=True)
    g0 = m.generation()
    m.eval()                                        # already in eval mode
    assert m.generation() == g0
    m.load_state_dict(_model(256, 16, 71).state_dict())
    g1 = m.generation()
    assert g1[0] != g0[0] and g1[1] != g0[1]        # adapter and inner model
    m.train()
    g2 = m.generation()
    assert g2 != g1
    m.train_step(torch.randn(16, 12, 256, device=DEV), torch.randn(16, 12, 256, device=DEV))
    assert m.generation()[0] != g2[0]               # the optimiser step
    m.eval()
    g3 = m.generation()
    m.rale.load_state_dict(m.rale.state_dict())
    assert m.generation()[1] != g3[1]


def test_two_graphed_forwards_on_one_model_replay_without_recapture():
    from ecg_denoise_amd.infer import GraphedForward
    m = _model(256, 16, 80, train=True)
    ga, gb = GraphedForward(m, 16), GraphedForward(m, 8)
    graphs = (ga.graph, gb.graph)
    x = torch.randn(16, 12, 256, device=DEV)
    for _ in range(3):
        ya = ga(x).clone()
        yb = gb(x[:8]).clone()
    assert (ga.graph, gb.graph) == graphs           # no call re-captured
    assert not m.training
    torch.cuda.synchronize()
    assert torch.equal(ya, m(x)) and torch.equal(yb, m(x[:8]))
    # a replay does not change the caller's mode: a model in training mode is refused, and stays in training mode
    m.train()
    with pytest.raises(_lib().RalError):
        ga(x)
    assert m.training
    m.eval()                                        # the mode flips twice: one re-capture per object, then replays
    ga(x); gb(x[:8])
    graphs = (ga.graph, gb.graph)
    ga(x); gb(x[:8])
    assert (ga.graph, gb.graph) == graphs


# ---------------------------------------------------------------------------------------------------------------------
# the back kernel at a window length that is a multiple of 16 only, with an odd half-overlap (partial 4-sample tiles at
# both ends of every kept range)
# ---------------------------------------------------------------------------------------------------------------------
def test_whole_record_off_grid_length_odd_half_overlap():
    from ecg_denoise_amd.infer import StreamingDenoiser
    L, ov = 400, 6
    hop, h = L - ov, ov // 2
    m = _model(L, 16, 90)
    T = 5000
    rec = _records(2, T, 12)
    sd = StreamingDenoiser(m, batch=16, overlap=ov, use_graph=False)
    starts = sd.window_starts(T)
    n = len(starts)
    assert n == sd.windows_per_record(T) and (T - L) % hop and 2 * n > 16
    out = sd.denoise(rec.to(DEV)).cpu()
    graphed = StreamingDenoiser(m, batch=16, overlap=ov, use_graph=True).denoise(rec.to(DEV)).cpu()
    assert torch.equal(out, graphed)
    # host reference: torch z-score, the eval model on the windows, de-normalise, keep-the-centre stitching
    want = torch.full_like(rec, float("nan"))
    for r in range(2):
        w = torch.stack([rec[r, :, s:s + L] for s in starts])
        mu = w.mean(-1, keepdim=True)
        sdv = w.std(-1, unbiased=False, keepdim=True).clamp_min(1e-6)
        yw = torch.cat([m(((w[i:i + 16] - mu[i:i + 16]) / sdv[i:i + 16]).to(DEV).contiguous()).cpu() for i in range(0, n, 16)])
        yw = yw * sdv + mu
        for k, s in enumerate(starts):
            a = 0 if k == 0 else h
            b = L if k == n - 1 else L - h
            if k == n - 1 and k > 0:
                a = max(h, starts[k - 1] + L - h - s)
            want[r, :, s + a:s + b] = yw[k, :, a:b]
    assert not torch.isnan(want).any()
    assert rel(out.numpy(), want.numpy()) <= 1e-5
