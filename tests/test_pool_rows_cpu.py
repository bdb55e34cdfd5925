"""The slot protocol is checked once for all stream pools (`slots_walk`, csrc/ral_slots.hpp): the same edit of a row's shared
fields - slot, turn, flags, x_off, T - is refused by every entry point that takes a table, with the same rule and the row that
breaks it.  No device: the pointers are dummies, and every call below is refused before anything is copied or launched (a sound
table is only ever sent with a launch argument, checked after the table, that is refused too).

x_off is not edited for the two emit entry points, `ral_pool_emit` and `ral_newrale_pool_back`: an emit has no chunks, so both
skip the chunk rule (one shared check, `pool_emit_fault`)."""
import ctypes as C

import numpy as np
import pytest

from ecg_denoise_amd import _lib
from ecg_denoise_amd.beats import BeatPoolState, _Detector
from ecg_denoise_amd.infer import PoolState
from ecg_denoise_amd.rate import RatePoolState, rate_ratio
from ecg_denoise_amd.rhythm import RhythmPoolState

FAKE = C.c_void_p(4096)        # non-null, never dereferenced
CAP = 4


def _two_pushes(st, first, second):
    """two streams that have `first` samples each and get `second` more; the second one ends -> the second call's table"""
    a, b = st.open(), st.open()
    st.commit(st.plan({a: (st.leads, first[0]), b: (st.leads, first[1])})[1])
    return st.plan({a: (st.leads, second[0]), b: (st.leads, second[1])}, close=(b,))[1]


def _window_pool(name, leads, grid):
    tab = _two_pushes(PoolState(CAP, leads, 256, 0, grid=grid), (300, 256), (300, 300))
    x_total, out_total, nw = int(tab["c"].sum()), int(tab["m"].sum()), int(tab["nw"].sum())
    lib = _lib.lib()

    def call(t, w0=0, nb=nw):
        p = t.ctypes.data
        if name == "ral_pool_windows":
            return lib.ral_pool_windows(FAKE, FAKE, x_total, p, len(t), FAKE, 1, CAP, leads, 256, 256, 1, w0, nb, FAKE, FAKE, None)
        if name == "ral_pool_emit":
            return lib.ral_pool_emit(FAKE, FAKE, p, len(t), FAKE, 1, CAP, leads, 256, 256, w0, nb, 0, FAKE, out_total, FAKE, FAKE,
                                     None)
        if name == "ral_newrale_pool_front":
            return lib.ral_newrale_pool_front(FAKE, FAKE, x_total, p, len(t), FAKE, 1, CAP, 256, 256, 1, w0, nb, FAKE, FAKE, FAKE,
                                              None)
        return lib.ral_newrale_pool_back(FAKE, FAKE, FAKE, p, len(t), FAKE, 1, CAP, 256, 256, w0, nb, 0, FAKE, out_total, FAKE, FAKE,
                                         None)
    return tab, call, (dict(w0=-1), "a window range")


def _rate_pool():
    up, down = rate_ratio(500, 360)
    st = RatePoolState(up, down, 2, CAP)
    tab = _two_pushes(st, (100, 40), (50, 30))

    def call(t):
        return _lib.lib().ral_rate_pool(FAKE, FAKE, int(tab["c"].sum()), t.ctypes.data, len(t), FAKE, 1, CAP, 2, up, down, FAKE,
                                        20 * max(up, down) + 1, st.hist_len, FAKE, int(tab["m"].sum()), None)
    return tab, call, None      # (nothing is checked after the table that a sound one could be refused for)


def _beat_pool():
    st = BeatPoolState(2, CAP)
    tab = _two_pushes(st, (900, 37), (500, 50))
    d = _Detector(360, 0.35, 0.0, (8, 24), 2, "cpu", "test")

    def call(t):
        return _lib.lib().ral_beat_pool(FAKE, FAKE, int(tab["c"].sum()), t.ctypes.data, len(t), FAKE, 1, CAP, 2, d.geom, FAKE,
                                        d.bank_host.size, st.hist_len, FAKE, 0, FAKE, int(tab["cap"].sum()), FAKE, None)
    return tab, call, ({}, "scratch")      # no scratch: the check behind the table's


def _rhythm_pool():
    st = RhythmPoolState(2, CAP)
    a, b = st.open(), st.open()
    btab = st.plan({a: (2, 900), b: (2, 37)})[1]
    st.beats.commit(btab)
    st.commit(st.table(btab, [3, 0]))
    tab = st.table(st.plan({a: (2, 500), b: (2, 50)}, close=(b,))[1], [7, 0])
    geom = _lib.RhythmGeom(36, 3, 0.7, 0.8)

    def call(t):
        return _lib.lib().ral_rhythm_pool(FAKE, FAKE, int(tab["c"].sum()), t.ctypes.data, len(t), FAKE, 1, CAP, 2, geom,
                                          st.beats.hist_len, FAKE, FAKE, FAKE, int(tab["m"].sum()), FAKE, 0, FAKE, FAKE, FAKE, FAKE,
                                          int(tab["ne"].sum()), None)
    return tab, call, ({}, "scratch")


POOLS = {
    "ral_pool_windows": lambda: _window_pool("ral_pool_windows", 2, (64, 2048)),
    "ral_pool_emit": lambda: _window_pool("ral_pool_emit", 2, (64, 2048)),
    "ral_newrale_pool_front": lambda: _window_pool("ral_newrale_pool_front", 12, (16, 1024)),
    "ral_newrale_pool_back": lambda: _window_pool("ral_newrale_pool_back", 12, (16, 1024)),
    "ral_rate_pool": _rate_pool,
    "ral_beat_pool": _beat_pool,
    "ral_rhythm_pool": _rhythm_pool,
}
T_RULE = ("T = n0 + c >= ", " without RAL_POOL_KEEP, or T = -1 with RAL_POOL_KEEP")


@pytest.mark.parametrize("entry", list(POOLS))
def test_every_table_entry_point_refuses_a_bad_slot_row(entry):
    tab, call, after = POOLS[entry]()
    who = entry[len("ral_"):]
    assert len(tab) == 2 and tab["T"][0] == -1 and tab["T"][1] == tab["n0"][1] + tab["c"][1] and tab["slot"].tolist() == [0, 1]
    assert tab["flags"].tolist() == [_lib.POOL_KEEP, 0]

    def refused(t, **kw):
        assert call(t, **kw) != 0
        return _lib.lib().ral_last_error().decode()

    if after is not None:      # the table as planned passes the walk: the refusal is for what comes after it
        msg = refused(tab.copy(), **after[0])
        assert msg.startswith(f"{who}: need ") and after[1] in msg and " in row" not in msg, msg

    either = [("slot", CAP, ("0 <= slot < capacity",)), ("slot", -1, ("0 <= slot < capacity",)), ("turn", 2, ("turn 0 or 1",)),
              ("flags", 2, ("flags RAL_POOL_KEEP or 0",))]
    if entry not in ("ral_pool_emit", "ral_newrale_pool_back"):
        either.append(("x_off", -1, ("the chunk inside the packed chunks",)))
    cases = [(r, f, v, rule) for r in (0, 1) for f, v, rule in either]
    cases += [(1, "slot", int(tab["slot"][0]), ("every slot at most once",)),
              (1, "T", int(tab["n0"][1] + tab["c"][1] + 1), T_RULE),      # the closing row: T beside n0 + c
              (1, "flags", _lib.POOL_KEEP, T_RULE),                       # the closing row kept
              (0, "flags", 0, T_RULE)]                                    # the open row not kept
    for r, field, value, rule in cases:
        t = tab.copy()
        t[field][r] = value
        msg = refused(t)
        assert msg.startswith(f"{who}: need ") and all(part in msg for part in rule) and f" in row {r} (" in msg, (r, field, value, msg)
