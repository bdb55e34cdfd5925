"""CPU-side checks of live streaming (LiveDenoiser, ral_live_windows / ral_live_emit): the entry points are exported, bad
arguments and null pointers are refused with a message before anything is launched (no GPU here: a launch would fail), and
a brute force over small windows confirms the host geometry the live path rests on: after n samples, [0, F(n)) is final
for every length the stream may end at, and the lag of a stream fed on the hop grid is D."""
import ctypes as C

import numpy as np
import pytest

from ecg_denoise_amd import _lib
from ecg_denoise_amd.infer import live_frontier, live_latency

NAMES = ("ral_live_windows", "ral_live_emit")


def _buf(n):
    a = np.zeros(n, dtype=np.float32)
    return a, C.c_void_p(a.ctypes.data)


def test_symbols_exported():
    L = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS, name


# ---- argument validation ----------------------------------------------------------------------------------------------
GOOD = dict(S=2, leads=2, L=256, hop=256, C=256, base=0, k0=1, nw=1, T=-1, w0=0, nb=2)

# every case must be refused by both entry points (a bad window range, stream geometry or batch)
BAD_BOTH = {
    "no_streams": dict(S=0),
    "no_leads": dict(leads=0),
    "L_not_multiple_of_64": dict(L=250, hop=250),
    "L_above_2048": dict(L=2112, hop=2112),
    "L_zero": dict(L=0, hop=0),
    "hop_zero": dict(hop=0),
    "hop_above_L": dict(hop=258),
    "odd_overlap": dict(hop=255),
    "T_shorter_than_L": dict(T=200),
    "k0_past_stream_end": dict(T=512, k0=2),           # a stream of 512 samples has windows 0 and 1
    "negative_k0": dict(k0=-1),
    "negative_w0": dict(w0=-1),
    "window_range_past_end": dict(w0=1, nb=2),          # S * nw = 2 windows
    "negative_nw": dict(nw=-1),
}
BAD_WINDOWS = {
    "window_before_history": dict(base=300),            # window 1 starts at 256, V at 300
    "window_past_chunk": dict(k0=1, nw=2),              # window 2 ends at 768, V = [0, 512)
    "negative_chunk": dict(C=-1),
    "nothing_to_do": dict(nb=0, hist_out=False),
}
BAD_EMIT = {
    "negative_lo": dict(lo=-1),
    "negative_m": dict(m=-1),
    "no_windows": dict(nb=0),
    "last_y_without_last_stats": dict(last="y"),
    "last_stats_without_last_y": dict(last="stats"),
}


def _windows(a, ptrs):
    hist, x, hist_out, win, stats = ptrs
    return _lib.lib().ral_live_windows(hist, x, hist_out if a.get("hist_out", True) else None, a["S"], a["leads"], a["L"],
                                       a["hop"], a["C"], a["base"], a["k0"], a["nw"], a["T"], a["w0"], a["nb"], win, stats, None)


def _emit(a, ptrs):
    y, stats, out, last_y, last_stats = ptrs
    last = a.get("last", "both")
    return _lib.lib().ral_live_emit(y, stats, a["S"], a["leads"], a["L"], a["hop"], a["k0"], a["nw"], a["T"], a["w0"], a["nb"],
                                    a.get("lo", 0), a.get("m", 256), out, last_y if last in ("both", "y") else None,
                                    last_stats if last in ("both", "stats") else None, None)


CASES = [("windows", c, v) for c, v in {**BAD_BOTH, **BAD_WINDOWS}.items()] + \
        [("emit", c, v) for c, v in {**BAD_BOTH, **BAD_EMIT}.items()]


@pytest.mark.parametrize("which,case,over", CASES, ids=[f"{w}-{c}" for w, c, _ in CASES])
def test_bad_arguments_are_refused(which, case, over):
    keep = [_buf(16) for _ in range(5)]            # valid host pointers; nothing may reach them
    ptrs = [p for _, p in keep]
    fn = _windows if which == "windows" else _emit
    rc = fn({**GOOD, **over}, ptrs)
    assert rc != 0, case
    msg = _lib.lib().ral_last_error().decode()
    assert f"live_{which}" in msg and "need" in msg, msg


@pytest.mark.parametrize("which,null_at", [("windows", i) for i in (0, 1, 3, 4)] + [("emit", i) for i in range(3)])
def test_null_pointers_are_refused(which, null_at):
    keep = [_buf(16) for _ in range(5)]
    ptrs = [p for _, p in keep]
    ptrs[null_at] = None
    fn = _windows if which == "windows" else _emit
    assert fn(dict(GOOD), ptrs) != 0
    assert f"live_{which}: null pointer" in _lib.lib().ral_last_error().decode()


# ---- host geometry: brute force against the offline stitch rule ---------------------------------------------------------
def _offline_owner(T, L, hop):
    """owner window and its start for every sample of a record of T samples: the rule of ral_stream_stitch
    (stream_keep / stream_owner in ral_stream.hip), restated on the host"""
    n_reg = (T - L) // hop + 1
    n = n_reg + (1 if (T - L) % hop else 0)
    h = (L - hop) // 2
    last_begin = (n - 2) * hop + L - h if n > 1 else 0
    owner = np.empty(T, dtype=np.int64)
    for t in range(T):
        if n == 1 or t >= last_begin:
            owner[t] = n - 1
        else:
            owner[t] = 0 if t < h else (t - h) // hop
    start = np.array([k * hop if k < n_reg else T - L for k in range(n)])
    return owner, start


@pytest.mark.parametrize("L", [8, 10, 12, 16])
def test_frontier_is_final_for_every_length(L):
    for overlap in range(0, L, 2):
        hop = L - overlap
        for n in range(L, 4 * L + 1):
            F = live_frontier(n, L, hop)
            assert F <= n
            owners = None
            for T in range(n, n + 2 * L + 2 * hop):
                owner, start = _offline_owner(T, L, hop)
                o = owner[:F]
                if owners is None:
                    owners = o
                    n_reg_n = (n - L) // hop + 1
                    assert np.all(o < n_reg_n), (L, hop, n)                           # a regular window complete at n
                    assert np.all(start[o] + L <= n), (L, hop, n)
                assert np.array_equal(o, owners), (L, hop, n, T)                     # the same owner for every T >= n
            if F < n:   # F(n) is the largest such frontier: sample F(n) belongs to a window that is not complete at n
                owner, start = _offline_owner(n + hop, L, hop)
                assert start[owner[F]] + L > n, (L, hop, n)
        assert live_frontier(L - 1, L, hop) == 0


@pytest.mark.parametrize("L", [8, 12, 64, 512])
def test_latency_on_the_hop_grid(L):
    for overlap in range(0, L, 2):
        hop = L - overlap
        D = live_latency(L, hop)
        assert D == (-L) % hop + (L - hop) // 2
        if overlap == 0:
            assert D == 0
        for n in range(0, 6 * L, hop):
            if n >= L:
                assert n - live_frontier(n, L, hop) == D, (L, hop, n)
                for c in (hop, 3 * hop):                     # a chunk on the hop grid emits exactly its length
                    assert live_frontier(n + c, L, hop) - live_frontier(n, L, hop) == c
