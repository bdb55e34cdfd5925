"""The stream pool for a 12-lead NewRALE (NewRALELivePool; ral_newrale_pool_front / _back): the cases of tests/test_gpu_pool.py
through the adapter kernels, at L = 1024 and at a window length off the 64-sample grid (L = 400).  Every comparison is bitwise."""
import pytest
import torch

from test_gpu_live import DEV, _lib, _p, _records, _s
from test_gpu_newrale_live import _model
from test_gpu_pool import (check_against_offline, check_frontier, check_lockstep, check_pool_emit_equals_stream_stitch,
                           check_pool_windows_equal_stream_windows, check_raising_calls, check_tenancy, make_schedule,
                           run_schedule)

pytestmark = pytest.mark.gpu


class Adapter:
    """ral_newrale_stream_front / _back and ral_newrale_pool_front / _back behind the calling convention of test_gpu_pool.Generic"""
    leads, inner = 12, 2

    def __init__(self, model):
        self.prm = model.params

    def windows_off(self, rec, T, L, hop, n):
        win = torch.full((n, 2, L), float("nan"), device=DEV)
        st = torch.full((n * 12 * 2,), float("nan"), device=DEV)
        _lib().check(_lib().lib().ral_newrale_stream_front(_p(rec), 1, T, L, hop, 0, n, _p(self.prm), _p(win), _p(st), _s()))
        return win, st

    def stitch_off(self, y, st, T, L, hop, n):
        out = torch.full((12, T), float("nan"), device=DEV)
        _lib().check(_lib().lib().ral_newrale_stream_back(_p(y), _p(st), _p(self.prm), 1, T, L, hop, 0, n, _p(out), _s()))
        return out

    def windows_pool(self, hist, xp, x_total, tab, tab_dev, upload, cap, L, hop, write_hist, w0, nb, win, st):
        return _lib().lib().ral_newrale_pool_front(_p(hist), _p(xp), x_total, tab.ctypes.data, len(tab), _p(tab_dev), upload, cap,
                                                   L, hop, write_hist, w0, nb, _p(self.prm), _p(win), _p(st), _s())

    def emit_pool(self, y, st, tab, tab_dev, upload, cap, L, hop, w0, nb, from_last, out, out_total, ly, ls):
        return _lib().lib().ral_newrale_pool_back(_p(y), _p(st), _p(self.prm), tab.ctypes.data, len(tab), _p(tab_dev), upload,
                                                  cap, L, hop, w0, nb, from_last, _p(out), out_total, _p(ly), _p(ls), _s())


@pytest.mark.parametrize("L,overlap", [(1024, 0), (1024, 34), (1024, 64), (400, 34)])
def test_pool_front_equals_stream_front_bitwise(L, overlap):
    check_pool_windows_equal_stream_windows(Adapter(_model(L)), L, overlap)


@pytest.mark.parametrize("L,overlap", [(1024, 0), (1024, 34), (1024, 64), (400, 34)])
def test_pool_back_equals_stream_back_bitwise(L, overlap):
    check_pool_emit_equals_stream_stitch(Adapter(_model(L)), L, overlap)


@pytest.mark.parametrize("L,overlap", [(1024, 128), (400, 6), (400, 0)])
def test_pool_equals_offline(L, overlap):
    from ecg_denoise_amd import NewRALELivePool
    m = _model(L)
    hop = L - overlap
    recs, calls = make_schedule(L, hop, 12, seed=9 + overlap, n_streams=12)
    pool = NewRALELivePool(m, capacity=5, overlap=overlap)
    assert (pool.capacity, pool.L, pool.hop, pool.leads) == (5, L, hop, 12)
    pieces = run_schedule(pool, recs, calls, device_chunks=True)
    check_frontier(pieces, calls, L, hop)
    check_against_offline(m, pieces, recs, overlap)


def test_a_stream_alone_equals_the_stream_in_the_crowd():
    from ecg_denoise_amd import NewRALELivePool
    m = _model(400)
    recs, calls = make_schedule(400, 400 - 34, 12, seed=41, n_streams=12)
    check_tenancy(lambda cap: NewRALELivePool(m, capacity=cap, overlap=34), recs, calls, 5)


def test_pool_in_lockstep_equals_live_denoiser():
    from ecg_denoise_amd import NewRALELiveDenoiser, NewRALELivePool
    m = _model(400)
    check_lockstep(m, lambda S, C: NewRALELiveDenoiser(m, S, C, 6), lambda S: NewRALELivePool(m, S, 6), 12, 400, 6)


def test_a_call_that_raises_changes_nothing():
    from ecg_denoise_amd import NewRALELivePool
    m = _model(400)
    recs, calls = make_schedule(400, 400 - 64, 12, seed=6, n_streams=8)
    check_raising_calls(m, NewRALELivePool(m, capacity=6, overlap=64), recs, calls, 64, 12, 400)


def test_training_mode_and_the_other_class_s_model_are_refused():
    from ecg_denoise_amd import LivePool, NewRALE, NewRALELivePool, RALENet
    RalError = _lib().RalError
    m = NewRALE(RALENet("full", leads=2, L=400, max_batch=8, train=True, device=DEV, seed=41), seed=42).eval()   # (trainable)
    with pytest.raises(RalError, match="NewRALELivePool"):
        LivePool(m, 4)
    with pytest.raises(RalError, match="LivePool takes"):
        NewRALELivePool(m.rale, 4)
    pool = NewRALELivePool(m, 2)
    sid = pool.open()
    rec = _records(1, 12, 900, 3)[0]
    a = pool.push({sid: rec[:, :500]})
    m.train()
    try:
        with pytest.raises(RalError, match="eval"):
            pool.push({sid: rec[:, 500:]})
        with pytest.raises(RalError, match="eval"):
            pool.close(sid)
        assert pool.samples_in(sid) == 500
    finally:
        m.eval()
    b = pool.close(sid, rec[:, 500:])
    check_against_offline(m, {0: [a[sid], b]}, [rec], 0)


def test_weights_changed_between_two_calls_are_used():
    """the adapter's and the inner model's weights replaced between two calls: the next call equals a pool that had the new
    weights from the start"""
    from ecg_denoise_amd import NewRALE, NewRALELivePool, RALENet
    L = 256
    mk = lambda seed: NewRALE(RALENet("full", leads=2, L=L, max_batch=8, train=False, device=DEV, seed=seed), seed=seed + 1).eval()
    m, other = mk(41), mk(77)
    rec = _records(2, 12, 6 * 360, 8)
    feed = lambda p, ids, i: p.push({sid: rec[s, :, i * 360:(i + 1) * 360] for s, sid in enumerate(ids)})
    pool = NewRALELivePool(m, 2, overlap=64)
    ids = [pool.open(), pool.open()]
    before = [feed(pool, ids, i) for i in range(3)]
    m.load_state_dict(other.state_dict())
    fresh = NewRALELivePool(other, 2, overlap=64)
    fids = [fresh.open(), fresh.open()]
    ref = [feed(fresh, fids, i) for i in range(6)]
    for i in range(3, 6):
        a = feed(pool, ids, i)
        torch.cuda.synchronize()
        assert all(torch.equal(a[x], ref[i][y]) for x, y in zip(ids, fids)), i
    assert any(not torch.equal(before[2][x], ref[2][y]) for x, y in zip(ids, fids))
