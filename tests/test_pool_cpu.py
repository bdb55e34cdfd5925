"""CPU-side checks of the stream pool (LivePool / NewRALELivePool; ral_pool_windows / ral_pool_emit, ral_newrale_pool_front /
_back): the entry points are exported, a bad table, bad geometry and null pointers are refused with a message before anything
is launched or copied (no GPU here: either would fail), a brute force over small windows confirms the host planner the pool
rests on (`pool_plan`), and the Python-side argument checks (`PoolState.plan`) refuse what the issue lists and change nothing."""
import ctypes as C

import numpy as np
import pytest

from ecg_denoise_amd import _lib
from ecg_denoise_amd.infer import PoolState, live_frontier, pool_plan
from test_live_cpu import _offline_owner

NAMES = ("ral_pool_windows", "ral_pool_emit", "ral_newrale_pool_front", "ral_newrale_pool_back")


def _buf(n):
    a = np.zeros(n, dtype=np.float32)
    return a, C.c_void_p(a.ctypes.data)


def test_symbols_exported():
    L = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS, name


def test_row_record_matches_the_header():
    """80 bytes: seven 64-bit fields, then six 32-bit ones, in the header's order"""
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ralenet.h")).read()
    body = re.search(r"typedef struct ral_pool_row \{(.*?)\} ral_pool_row;", hdr, re.S).group(1)
    fields = re.findall(r"(int64_t|int32_t)\s+(\w+);", body)
    assert [n for _, n in fields] == list(_lib.POOL_ROW.names)
    assert [t for t, _ in fields] == ["int64_t" if _lib.POOL_ROW[n].itemsize == 8 else "int32_t" for n in _lib.POOL_ROW.names]
    assert _lib.POOL_ROW.itemsize == 80
    assert int(re.search(r"#define RAL_POOL_KEEP (\d+)", hdr).group(1)) == _lib.POOL_KEEP


# ---- argument validation ----------------------------------------------------------------------------------------------
# (tests/test_gpu_pool.py launches this table as it stands: every refusal below is for the one edit its case makes)
# two streams, overlap 0, L = hop = 256.  Row 0: slot 0 had 300 samples and gets 300 more, stays open: window 1 = [256, 512)
# becomes complete (V = [44, 600)), samples [256, 512) become final.  Row 1: slot 3 had 256 samples, gets 300 and ends at
# T = 556: windows 1 = [256, 512) and 2 = [300, 556) (right-aligned), samples [256, 556).
def _good_rows():
    t = np.zeros(2, dtype=_lib.POOL_ROW)
    t[0] = (300, -1, 1, 256, 0, 0, 0, 0, 300, 1, 256, 0, _lib.POOL_KEEP)
    t[1] = (256, 556, 1, 256, 300, 256, 1, 3, 300, 2, 300, 1, 0)
    return t


GOOD = dict(capacity=4, leads=2, L=256, hop=256, x_total=600, out_total=556, w0=0, nb=3, write_hist=1, from_last=0)


def _row(r, **kw):
    def edit(t):
        for k, v in kw.items():
            t[k][r] = v
    return edit


# every case: (the edit, the rule the message must name).  BAD_BOTH must be refused by all four entry points (for the 12-lead
# pair with leads = 12 throughout), and each for the rule its edit breaks - no other check may fire first
BAD_BOTH = {
    "slot_out_of_range": (_row(1, slot=4), "0 <= slot < capacity in row 1"),
    "negative_slot": (_row(0, slot=-1), "0 <= slot < capacity in row 0"),
    "duplicate_slot": (_row(1, slot=0), "every slot at most once in row 1"),
    "k_past_the_end_of_a_closed_stream": (_row(1, nw=3), "windows k0 .. k0 + nw - 1 in the stream in row 1"),   # 556 samples: windows 0, 1, 2
    "T_shorter_than_L": (_row(1, n0=0, c=200, T=200, k0=0, nw=1, lo=0, m=200), "T = n0 + c >= L"),
    "T_is_not_n0_plus_c": (_row(1, T=600), "T = n0 + c >= L"),
    "open_row_without_keep": (_row(0, flags=0), "T = -1 with RAL_POOL_KEEP"),
    "open_row_without_samples": (_row(0, c=0, nw=0, m=0), "T = -1 with RAL_POOL_KEEP and c >= 1 in row 0"),
    "closing_row_with_keep": (_row(1, flags=_lib.POOL_KEEP), "without RAL_POOL_KEEP"),
    "turn_out_of_range": (_row(0, turn=2), "turn 0 or 1 in row 0"),
    "w_off_is_not_the_prefix": (_row(1, w_off=2), "w_off the prefix sum of nw in row 1"),
    "negative_n0": (_row(0, n0=-1), "n0, c, nw, m, k0, lo >= 0"),
    "odd_overlap": (dict(hop=255), "L - hop even"),
    "L_off_the_grid": (dict(L=250, hop=250), "L a multiple of"),
    "L_too_long": (dict(L=2112, hop=2112), "L a multiple of"),
    "hop_above_L": (dict(hop=258), "1 <= hop <= L"),
    "zero_rows": (dict(rows=0), "rows >= 1"),
    "zero_capacity": (dict(capacity=0), "capacity >= 1"),
    "negative_w0": (dict(w0=-1), "a window range"),
    "window_range_past_the_call": (dict(w0=2, nb=2), "a window range"),
    "more_emitted_than_received": (_row(0, m=400), "lo + m <= n0 + c"),                   # lo + m = 656 > n0 + c = 600
}
BAD_WINDOWS = {
    # V = [344, 900) and window 1 starts at 256; lo + m = 512 stays inside the received samples, so only this rule is broken
    "window_before_the_history": (_row(0, n0=600), "the first window at or after the history, max(n0 - L, 0) in row 0"),
    "window_past_the_chunk": (_row(0, nw=2), "the last window inside the received samples, n0 + c in row 0"),   # ends at 768 > 600
    "chunk_past_the_packed_buffer": (dict(x_total=599), "the chunk inside the packed chunks in row 1"),
    "negative_chunk_offset": (_row(0, x_off=-1), "the chunk inside the packed chunks in row 0"),
    "negative_chunk": (_row(0, c=-1), "n0, c, nw, m, k0, lo >= 0"),
    "nothing_to_do": (dict(nb=0, write_hist=0), "nb >= 1 or write_hist"),
}
BAD_EMIT = {
    "output_past_the_packed_buffer": (dict(out_total=555), "the emitted samples inside the packed output in row 1"),
    "negative_output_offset": (_row(0, out_off=-1), "the emitted samples inside the packed output in row 0"),
    "negative_m": (_row(0, m=-1), "n0, c, nw, m, k0, lo >= 0"),
    "lo_before_the_windows": (_row(0, lo=200), "[lo, lo + m) inside the windows in row 0"),
    "no_windows": (dict(nb=0), "a window range of nb >= 1"),
    "last_y_without_last_stats": (dict(last="y"), "both given or both null"),
    "last_stats_without_last_y": (dict(last="stats"), "both given or both null"),
    "from_last_with_a_regular_table": (dict(from_last=1, last="none"), "from_last rows with T known"),
}


def _call(which, a, tab, ptrs):
    """ptrs: hist / y, x / stats, table_dev, win / out, stats / last_y, last_stats, adapter parameters"""
    lib = _lib.lib()
    p0, p1, tdev, p3, p4, p5, prm = ptrs
    table = C.c_void_p(tab.ctypes.data) if a.get("table", True) else None
    rows = a.get("rows", len(tab))
    if which == "pool_windows":
        return lib.ral_pool_windows(p0, p1, a["x_total"], table, rows, tdev, 1, a["capacity"], a["leads"], a["L"], a["hop"],
                                    a["write_hist"], a["w0"], a["nb"], p3, p4, None)
    if which == "newrale_pool_front":
        return lib.ral_newrale_pool_front(p0, p1, a["x_total"], table, rows, tdev, 1, a["capacity"], a["L"], a["hop"],
                                          a["write_hist"], a["w0"], a["nb"], prm, p3, p4, None)
    last = a.get("last", "both")
    ly, ls = (p4 if last in ("both", "y") else None), (p5 if last in ("both", "stats") else None)
    if which == "pool_emit":
        return lib.ral_pool_emit(p0, p1, table, rows, tdev, 1, a["capacity"], a["leads"], a["L"], a["hop"], a["w0"], a["nb"],
                                 a["from_last"], p3, a["out_total"], ly, ls, None)
    return lib.ral_newrale_pool_back(p0, p1, prm, table, rows, tdev, 1, a["capacity"], a["L"], a["hop"], a["w0"], a["nb"],
                                     a["from_last"], p3, a["out_total"], ly, ls, None)


GATHER, EMIT = ("pool_windows", "newrale_pool_front"), ("pool_emit", "newrale_pool_back")
CASES = [(w, c, v, e) for w in GATHER for c, (v, e) in {**BAD_BOTH, **BAD_WINDOWS}.items()] + \
        [(w, c, v, e) for w in EMIT for c, (v, e) in {**BAD_BOTH, **BAD_EMIT}.items()]


def _args(which, over):
    a, tab = dict(GOOD), _good_rows()
    if "newrale" in which:
        a["leads"] = 12
    if callable(over):
        over(tab)
    else:
        a.update(over)
    if "newrale" in which and a["L"] == 2112:      # the 12-lead pair ends at L = 1024
        a["L"] = a["hop"] = 1040
    return a, tab


@pytest.mark.parametrize("which,case,over,expect", CASES, ids=[f"{w}-{c}" for w, c, _, _ in CASES])
def test_bad_tables_and_geometry_are_refused(which, case, over, expect):
    keep = [_buf(16) for _ in range(7)]            # valid host pointers; nothing may reach them
    a, tab = _args(which, over)
    rc = _call(which, a, tab, [p for _, p in keep])
    assert rc != 0, case
    msg = _lib.lib().ral_last_error().decode()
    assert msg.startswith(f"{which}: need") and expect in msg, msg
    assert all(not b.any() for b, _ in keep)


def test_a_table_of_kept_windows_is_checked():
    """from_last: one window per row, the last regular window complete at n0, of a stream that ends; nothing is kept by such
    an emit.  The unedited table is refused only for keeping (its rows pass), every edit for the rows' rule"""
    t = np.zeros(1, dtype=_lib.POOL_ROW)
    # overlap 64 (hop 192): 448 samples, closed without a chunk; window 1 = [192, 448) is the last one and keeps [416, 448)
    t[0] = (448, 448, 1, 416, 0, 0, 0, 2, 0, 1, 32, 0, 0)
    for which in EMIT:
        base = dict(GOOD, hop=192, from_last=1, nb=1, out_total=32, leads=12 if "newrale" in which else 2)
        keep = [_buf(16) for _ in range(7)]
        assert _call(which, dict(base, last="both"), t.copy(), [p for _, p in keep]) != 0
        msg = _lib.lib().ral_last_error().decode()
        assert msg.startswith(f"{which}: need last_y and last_stats null with from_last"), msg
        for edit in (dict(k0=0), dict(k0=2), dict(nw=2), dict(n0=100, T=448, c=348), dict(T=-1, flags=_lib.POOL_KEEP, c=1)):
            bad = t.copy()
            for k, v in edit.items():
                bad[k][0] = v
            if "nw" in edit:
                base = dict(base, nb=1)
            assert _call(which, dict(base, last="none"), bad, [p for _, p in keep]) != 0, edit
            msg = _lib.lib().ral_last_error().decode()
            assert msg.startswith(f"{which}: need from_last rows with T known") and "in row 0" in msg, (edit, msg)
        assert all(not b.any() for b, _ in keep)


NULLS = [(w, i) for w in GATHER for i in (0, 1, 2, 3, 4)] + [(w, i) for w in EMIT for i in (0, 1, 2, 3)] + \
        [("newrale_pool_front", 6), ("newrale_pool_back", 6)] + [(w, "table") for w in GATHER + EMIT]


@pytest.mark.parametrize("which,null_at", NULLS)
def test_null_pointers_are_refused(which, null_at):
    keep = [_buf(16) for _ in range(7)]
    ptrs = [p for _, p in keep]
    a, tab = _args(which, {})
    if null_at == "table":
        a["table"] = False
    else:
        ptrs[null_at] = None
    assert _call(which, a, tab, ptrs) != 0
    assert f"{which}: null pointer" in _lib.lib().ral_last_error().decode()


# ---- the host planner: brute force against the offline stitch rule ------------------------------------------------------
def _chunkings(rng, T, L, count):
    """random cuts of [0, T) with chunk lengths from 1 to 2 L + 1 and beyond, c = 1 and c > 2 L included"""
    for i in range(count):
        cuts, n = [], 0
        while n < T:
            kind = rng.integers(0, 4)
            c = 1 if kind == 0 else int(rng.integers(2 * L + 1, 3 * L + 2)) if kind == 1 else int(rng.integers(1, 2 * L + 2))
            c = min(c, T - n)
            cuts.append(c)
            n += c
        yield cuts


@pytest.mark.parametrize("L", [8, 10, 12, 16])
def test_planner_tiles_every_stream_once_with_the_offline_owners(L):
    rng = np.random.default_rng(L)
    for overlap in range(0, L, 2):
        hop = L - overlap
        for T in list(range(L, L + 2 * hop + 1)) + [int(v) for v in rng.integers(L, 7 * L, size=6)]:
            owner, start = _offline_owner(T, L, hop)
            for cuts in _chunkings(rng, T, L, 4):
                # a stream may also end without a last chunk: the close is then a call of its own with c = 0
                if rng.integers(0, 2):
                    calls = [(c, False) for c in cuts] + [(0, True)]
                else:
                    calls = [(c, False) for c in cuts[:-1]] + [(cuts[-1], True)]
                n, emitted, kept_last = 0, 0, None
                for c, closing in calls:
                    k0, nw, lo, m, Tc = (int(v) for v in pool_plan(n, c, closing, L, hop))
                    assert Tc == (T if closing else -1)
                    assert lo == emitted, (L, hop, T, cuts)                                   # in order, nothing twice
                    assert k0 == ((n - L) // hop + 1 if n >= L else 0) and nw >= 0
                    wins = list(range(k0, k0 + nw))
                    for k in wins:                                                            # inside (last L samples ++ chunk)
                        st = k * hop if not closing or k < (T - L) // hop + 1 else T - L
                        assert st >= max(n - L, 0) and st + L <= n + c, (L, hop, T, cuts, k)
                        if closing:
                            assert st == start[k]
                    allowed = set(wins) | ({kept_last} if kept_last is not None else set())
                    own = owner[lo:lo + m]
                    assert set(own.tolist()) <= allowed, (L, hop, T, cuts, n, c)
                    if not closing:
                        assert np.all(start[own] == own * hop)                                # regular windows, as the open rule has them
                        assert n + c - (lo + m) == n + c - live_frontier(n + c, L, hop)       # held back: n - F(n)
                        if nw:
                            kept_last = k0 + nw - 1
                    n, emitted = n + c, lo + m
                assert n == T and emitted == T, (L, hop, T, cuts)


def test_planner_is_elementwise():
    n0, c, cl = np.array([0, 300, 256, 512]), np.array([100, 300, 300, 0]), np.array([False, False, True, True])
    got = pool_plan(n0, c, cl, 256, 256)
    for i in range(4):
        one = pool_plan(int(n0[i]), int(c[i]), bool(cl[i]), 256, 256)
        assert [int(g[i]) for g in got] == [int(v) for v in one]
    assert [int(g[1]) for g in got] == [1, 1, 256, 256, -1]
    assert [int(g[2]) for g in got] == [1, 2, 256, 300, 556]


# ---- Python-side refusals (no device) -----------------------------------------------------------------------------------
def test_state_refuses_bad_geometry():
    for overlap in (-2, 3, 256, 300):
        with pytest.raises(_lib.RalError, match="overlap"):
            PoolState(4, 2, 256, overlap)
    with pytest.raises(_lib.RalError, match="capacity"):
        PoolState(0, 2, 256, 0)
    for L in (400, 32, 2112):                    # off the generic kernels' grid
        with pytest.raises(_lib.RalError, match="multiple of 64 up to 2048"):
            PoolState(4, 2, L, 0)
    PoolState(4, 12, 400, 0, grid=(16, 1024))     # the 12-lead kernels take it
    for L in (408, 1040):
        with pytest.raises(_lib.RalError, match="multiple of 16 up to 1024"):
            PoolState(4, 12, L, 0, grid=(16, 1024))


def _snapshot(st):
    return st.n.copy(), st.turn.copy(), st.is_open.copy(), list(st.free)


def test_state_refusals_change_nothing():
    st = PoolState(3, 2, 256, 64)
    a, b = st.open(), st.open()
    sids, tab, last = st.plan({a: (2, 300), b: (2, 10)})
    st.commit(tab)
    before = _snapshot(st)
    bad = [
        (({2: (2, 10)}, ()), "not an open stream"),                 # never opened
        (({7: (2, 10)}, ()), "not an open stream"),                 # out of range
        (({"a": (2, 10)}, ()), "not an open stream"),
        (({a: (2, 10)}, (2,)), "not an open stream"),               # closing an unknown one
        (({a: (1, 10)}, ()), "expected a chunk of shape"),          # wrong lead count
        (({a: (2, 10, 1)}, ()), "expected a chunk of shape"),
        (({a: (2, 0)}, ()), "empty chunk"),                         # empty without close
        (({b: (2, 100)}, (b,)), "shorter than one window"),         # 10 + 100 < 256
        (({a: (2, 1)}, (b,)), "shorter than one window"),           # closing b at 10 samples
        (({}, ()), "nothing to do"),
    ]
    for (shapes, close), msg in bad:
        with pytest.raises(_lib.RalError, match=msg):
            st.plan(shapes, close)
        after = _snapshot(st)
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
    c = st.open()
    with pytest.raises(_lib.RalError, match="all 3 slots"):
        st.open()
    # the streams go on: a closes with a chunk, b is pushed, and a's slot is free again
    sids, tab, last = st.plan({a: (2, 212), b: (2, 246)}, close=(a,))
    assert sids == [a, b] and tab["T"].tolist() == [512, -1] and tab["flags"].tolist() == [0, _lib.POOL_KEEP]
    st.commit(tab)
    assert not st.is_open[a] and st.n[b] == 256 and st.open() == a and st.n[a] == 0
    with pytest.raises(_lib.RalError, match="not an open stream"):
        st.plan({c: (2, 5)}, close=(5,))


def test_state_tables_pass_the_library_checks():
    """the table `PoolState.plan` builds for a mixed call (chunks of 1 to 771 samples, three streams closing, one of them
    without a chunk) sizes the packed buffers exactly: one sample less of either is refused (the GPU tests run such tables)"""
    st = PoolState(8, 2, 256, 34)
    ids = [st.open() for _ in range(5)]
    _, tab, _ = st.plan({ids[0]: (2, 300), ids[1]: (2, 7), ids[2]: (2, 256), ids[3]: (2, 1000)})
    st.commit(tab)
    sids, tab, last = st.plan({ids[0]: (2, 1), ids[1]: (2, 360), ids[3]: (2, 771), ids[4]: (2, 256)}, close=(ids[2], ids[3], ids[4]))
    assert len(last) == 1 and last["slot"][0] == ids[2] and last["k0"][0] == 0
    keep = [_buf(16) for _ in range(7)]
    a = dict(GOOD, capacity=8, hop=222, x_total=int(tab["c"].sum()) - 1, out_total=int(tab["m"].sum()), nb=1)
    assert _call("pool_windows", a, tab, [p for _, p in keep]) != 0
    assert "need" in _lib.lib().ral_last_error().decode()
    a = dict(GOOD, capacity=8, hop=222, x_total=int(tab["c"].sum()), out_total=int(tab["m"].sum()) - 1, nb=1)
    assert _call("pool_emit", a, tab, [p for _, p in keep]) != 0
    assert "need" in _lib.lib().ral_last_error().decode()


def test_pools_refuse_the_other_class_s_model_without_a_device():
    """the model check comes first and needs no device: a stand-in that is not a NewRALE"""
    from ecg_denoise_amd import NewRALELivePool
    with pytest.raises(_lib.RalError, match="LivePool takes the 1- and 2-lead"):
        NewRALELivePool(object(), 4)
