"""The two ways `pack_chunks` brings a call's chunks to the device give every pool the same bytes: one push to three streams with
a host float64 array, a host float32 tensor and a device float32 tensor (copied chunk by chunk) against the same push with
three device float32 tensors (one `torch.cat`), then all three streams closed without a chunk (an empty pack).  The results
are compared bit for bit (floats as their int32 patterns: an RR ratio may be NaN), and so is everything the pools keep."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L, OVERLAP = 64, 16
BEAT_LENS = (700, 900, 1500)                      # the detector's lag is 657 samples at 360 Hz
LIVE_LENS = (L + 1, L + (L - OVERLAP), 2 * L)     # one window and a sample, one window and a hop, two windows


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _flat(res):
    """the results of a call -> [(sid, tensors)]"""
    return [(sid, tuple(_bits(t) for t in (r if isinstance(r, tuple) else (r,)))) for sid, r in res.items()]


def _equal(a, b):
    assert len(a) == len(b)
    for (sa, ta), (sb, tb) in zip(a, b):
        assert sa == sb and len(ta) == len(tb)
        for u, v in zip(ta, tb):
            assert u.dtype == v.dtype and u.shape == v.shape and torch.equal(u, v)


def _kept(pool, slots, tensors):
    """what a pool keeps between calls -> (host arrays, device tensors)"""
    host = [slots.n, slots.turn, slots.is_open, np.asarray(slots.free)]
    return host, [_bits(getattr(pool, t)) for t in tensors]


def _live():
    from ecg_denoise_amd import LivePool, RALENet
    model = RALENet("full", leads=2, L=L, max_batch=16, train=False, device=DEV, seed=11).eval()
    rec = torch.randn(3, 2, 2 * L, generator=torch.Generator().manual_seed(3)).numpy()
    mk = lambda: LivePool(model, 3, overlap=OVERLAP)
    return mk, rec, LIVE_LENS, lambda p: _kept(p, p.state, ("hist", "last_y", "last_stats"))


def _rate():
    from ecg_denoise_amd import ResamplerPool
    rec = torch.randn(3, 2, 2 * L, generator=torch.Generator().manual_seed(4)).numpy()
    return (lambda: ResamplerPool(500, 360, 2, 3, device=DEV)), rec, LIVE_LENS, lambda p: _kept(p, p.state, ("hist",))


def _beat_records():
    from ecg_denoise_amd import synth
    return synth.make_records_with_beats(3, 2, max(BEAT_LENS), seed=5)[0]


def _beats():
    from ecg_denoise_amd import BeatPool
    return (lambda: BeatPool(2, 3, 360, device=DEV)), _beat_records(), BEAT_LENS, lambda p: _kept(p, p.state, ("hist",))


def _classes():
    from ecg_denoise_amd import BeatClassPool

    def kept(p):
        host, dev = _kept(p, p.beats.state, ("ring", "ring_pos"))
        return host + [p.state.nb, p.state.done], dev + [_bits(p.beats.hist)]
    return (lambda: BeatClassPool(2, 3, 360, device=DEV)), _beat_records(), BEAT_LENS, kept


@pytest.mark.parametrize("case", [_live, _rate, _beats, _classes], ids=["LivePool", "ResamplerPool", "BeatPool", "BeatClassPool"])
def test_mixed_chunks_and_device_chunks_give_the_same(case):
    make, rec, lens, kept = case()

    def same_state(p, q):
        (hp, dp), (hq, dq) = kept(p), kept(q)
        assert all(np.array_equal(u, v) for u, v in zip(hp, hq)) and all(torch.equal(u, v) for u, v in zip(dp, dq))
    assert rec.dtype == np.float32 and rec.shape[0] == 3
    mixed, cat = make(), make()
    sids = [mixed.open() for _ in range(3)]
    assert [cat.open() for _ in range(3)] == sids == [0, 1, 2]
    x = [np.ascontiguousarray(r[:, :n]) for r, n in zip(rec, lens)]
    res_m = mixed.push({sids[0]: x[0].astype(np.float64), sids[1]: torch.from_numpy(x[1]), sids[2]: torch.from_numpy(x[2]).to(DEV)})
    res_c = cat.push({sid: torch.from_numpy(v).to(DEV) for sid, v in zip(sids, x)})
    first = _flat(res_m)
    assert any(t[0].numel() for _, t in first) or case is _classes      # (a stream's first eight classes wait for the ninth beat)
    _equal(first, _flat(res_c))
    same_state(mixed, cat)
    for pool in (mixed, cat):
        assert [pool.samples_in(s) for s in sids] == list(lens)
    rest_m, rest_c = _flat(mixed.push({}, close=sids)), _flat(cat.push({}, close=sids))
    assert any(t[0].numel() for _, t in rest_m)
    _equal(rest_m, rest_c)
    same_state(mixed, cat)
    assert mixed.open_streams == cat.open_streams == ()
