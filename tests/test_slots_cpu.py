"""What the stream pools share on the host (`ecg_denoise_amd.pools`), without a device: the slot table, the shared argument
checks in their order, the three state classes on top of it, and the packing of a call's chunks into one buffer."""
import numpy as np
import pytest
import torch

from ecg_denoise_amd import RalError, _lib
from ecg_denoise_amd.beats import BeatPoolState
from ecg_denoise_amd.infer import PoolState
from ecg_denoise_amd.pools import SlotState, as_chunks, pack_chunks
from ecg_denoise_amd.rate import RatePoolState


def _snap(st):
    return st.n.copy(), st.turn.copy(), st.is_open.copy(), list(st.free)


def _same(st, snap):
    return all(np.array_equal(u, v) for u, v in zip(_snap(st)[:3], snap[:3])) and st.free == snap[3]


def test_slots_are_handed_out_in_order_and_reused():
    st = SlotState(3, 2, "Pool")
    assert (st.n.dtype, st.turn.dtype, st.is_open.dtype, st.free) == (np.int64, np.int32, np.bool_, [2, 1, 0])
    assert [st.open(), st.open(), st.open()] == [0, 1, 2]
    with pytest.raises(RalError, match=r"Pool\.open: all 3 slots"):
        st.open()
    tab = np.zeros(2, dtype=[("slot", "<i4"), ("n0", "<i8"), ("c", "<i4"), ("flags", "<i4")])
    tab["slot"], tab["n0"], tab["c"], tab["flags"] = [1, 2], [0, 0], [5, 9], [0, _lib.POOL_KEEP]
    st.commit_rows(tab)
    assert st.n.tolist() == [0, 5, 9] and st.turn.tolist() == [0, 0, 1] and st.is_open.tolist() == [True, False, True]
    assert st.free == [1]
    tab["slot"], tab["n0"], tab["flags"] = [0, 2], [0, 9], [_lib.POOL_KEEP, 0]
    st.commit_rows(tab, flip=False)
    assert st.n.tolist() == [5, 5, 18] and st.turn.tolist() == [0, 0, 1] and st.free == [1, 2]      # closed rows, in table order
    assert st.open() == 2 and st.n[2] == 0                 # a closed slot is reused, its counter starts again
    for bad in (True, -1, 3, 1.0, 1, "0", None):           # 1 is a closed slot
        assert not st._is_open(bad)
    assert st._is_open(0) and st._is_open(np.int64(2)) and st._is_open(np.int32(0))
    for cap in (0, -1, True, 2.0, 2.5, "3", None):
        with pytest.raises(RalError, match="Pool: capacity must be >= 1"):
            SlotState(cap, 2, "Pool")


def test_named_refuses_in_the_shared_order_and_changes_nothing():
    st = SlotState(3, 2, "Pool")
    a, b = st.open(), st.open()
    st.n[a] = 11
    snap = _snap(st)
    for shapes, close, kw, what in (
            ({}, (), {}, r"Pool\.push: nothing to do"),
            ({a: (3, 5), 2: (2, 5)}, (), {}, r"Pool\.push: 2 is not an open stream"),                  # before the shape of a
            ({a: (2, 5)}, (True,), {}, r"Pool\.push: True is not an open stream"),
            ({a: (3, 5), b: (2, 5)}, (), {"max_rows": 1, "rows_what": "1 streams"},
             r"Pool\.push: more than 1 streams in one call"),                                          # before the shape of a
            ({a: (2, 5), b: (3, 1 << 30)}, (), {}, r"Pool\.push: stream 1: expected a chunk of shape \(2, samples\), got \(3, "),
            ({a: (5,)}, (), {}, r"Pool\.push: stream 0: expected a chunk of shape \(2, samples\), got \(5,\)"),
            ({a: (2, 1 << 30)}, (), {}, r"Pool\.push: a chunk of more than 2\^30 - 1 samples")):
        with pytest.raises(RalError, match=what):
            st.named(shapes, close, **kw)
        assert _same(st, snap)
    sids, slot, lens, ends, n0 = st.named({b: (2, (1 << 30) - 1)}, (a, b, a), max_rows=2, rows_what="2 streams")
    assert sids == [b, a] and slot.tolist() == [b, a] and lens.tolist() == [(1 << 30) - 1, 0] and ends.tolist() == [True, True]
    assert n0.tolist() == [0, 11] and slot.dtype == lens.dtype == n0.dtype == np.int64 and _same(st, snap)
    assert st.named({a: (2, 0)}, ())[3].tolist() == [False]


@pytest.mark.parametrize("make", [lambda: PoolState(3, 2, 256, 0), lambda: RatePoolState(18, 25, 2, 3),
                                  lambda: BeatPoolState(2, 3, 360)], ids=["PoolState", "RatePoolState", "BeatPoolState"])
def test_the_state_classes_share_the_slot_table(make):
    st = make()
    assert isinstance(st, SlotState) and "plan" in vars(type(st)) and not hasattr(SlotState, "plan")
    assert type(st).open is SlotState.open and type(st).named is SlotState.named and type(st)._is_open is SlotState._is_open
    assert (st.capacity, st.leads, st.free) == (3, 2, [2, 1, 0])
    a = st.open()
    with pytest.raises(RalError, match=rf"{st.name}\.push: 1 is not an open stream"):
        st.plan({a: (2, 300), 1: (2, 300)})
    sids, tab = st.plan({a: (2, 300)})[:2]
    st.commit(tab)
    assert sids == [a] and st.n.tolist() == [300, 0, 0] and st.turn.tolist() == [1, 0, 0]


def test_pack_chunks_on_the_host():
    rng = np.random.default_rng(3)
    x64 = rng.standard_normal((2, 5))
    xs = as_chunks({4: x64, 0: torch.zeros(2, 0, dtype=torch.float32),
                    2: torch.from_numpy(rng.standard_normal((2, 3)).astype(np.float32))})
    assert xs[4].dtype == torch.float32 and xs[2].dtype == torch.float32
    xp, x_total, views = pack_chunks(xs, 2, "cpu")
    assert x_total == 8 and xp.dtype == torch.float32 and xp.numel() == 16
    want = torch.cat([torch.from_numpy(x64.astype(np.float32)).reshape(-1), xs[0].reshape(-1), xs[2].reshape(-1)])
    assert torch.equal(xp[:x_total * 2], want)
    assert list(views) == [4, 0, 2]
    for (sid, v), off in zip(views.items(), (0, 10, 10)):
        assert tuple(v.shape) == (2, xs[sid].shape[1]) and torch.equal(v, xs[sid])
        assert v.untyped_storage().data_ptr() == xp.untyped_storage().data_ptr() and v.storage_offset() == off
    views[2][1, 2] = 7.0
    assert xp[15] == 7.0
    # a mixture of dtypes among host chunks goes the same way
    xp2, n2, _ = pack_chunks({1: torch.from_numpy(x64), 5: xs[2]}, 2, "cpu")
    assert n2 == 8 and torch.equal(xp2, torch.cat([want[:10], xs[2].reshape(-1)]))
    xp0, n0, v0 = pack_chunks({}, 2, "cpu")
    assert n0 == 0 and xp0.numel() == 2 and xp0.dtype == torch.float32 and v0 == {}
