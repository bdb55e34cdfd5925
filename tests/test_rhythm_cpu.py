"""Beat classes without a device: the geometry, the neighbourhood rule, the synthetic rhythm records, the oracle on them (and
the guard that makes the exact label comparison of tests/test_gpu_rhythm.py legitimate), the pool's planning and the ABI."""
import ctypes
import os
import re

import numpy as np
import pytest

import rhythm_util as U
import ecg_denoise_amd
from ecg_denoise_amd import RalError, _lib, rhythm_check, rhythm_geometry, synth
from ecg_denoise_amd.rhythm import RhythmPoolState, hood

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_geometry_and_supported_rates():
    assert rhythm_geometry(360) == {"Wb": 36, "Sa": 3}
    assert rhythm_geometry(500) == {"Wb": 50, "Sa": 4}            # 4.17 rounds down
    assert rhythm_geometry(250) == {"Wb": 25, "Sa": 2}            # 2.08
    assert rhythm_geometry(180) == {"Wb": 18, "Sa": 2}            # 1.5 rounds up
    for fs in (360, 500, 250, 128, 1000):
        assert rhythm_geometry(fs) == U.geometry(fs)
    for fs, leads in ((360, 1), (360, 51), (500, 12), (1000, 2), (1450, 2)):
        assert rhythm_check(fs, leads) == rhythm_geometry(fs)
    for fs, leads in ((360, 0), (360, True), (360, 70000), (4000, 2), (8000, 2)):
        with pytest.raises(RalError):
            rhythm_check(fs, leads)
    with pytest.raises(RalError):
        rhythm_geometry(359.5)


@pytest.mark.parametrize("n", [0, 1, 3, 4, 8, 9, 10, 30])
def test_neighbourhood_rule(n):
    for i in range(n):
        a, hi = hood(i, n)
        assert (a, hi) == U.hood(i, n)
        nb = [j for j in range(a, hi) if j != i]
        assert a <= i < hi and len(nb) == min(n - 1, 8)
        if i >= 8:
            assert nb == list(range(i - 8, i))                    # the eight beats before i
        elif n >= 9:
            assert nb == [j for j in range(9) if j != i]          # the first eight serve each other, with beat 8
        else:
            assert nb == [j for j in range(n) if j != i]          # a short record: all the others
        assert i == 0 or a <= i - 1                               # the beat before i is in the set that gives the median interval
    if n:
        assert hood(0, n) == (0, min(n, 9)) and hood(n - 1, n) == (max(0, n - 9), n)


def test_oracle_on_hand_made_beats():
    """the formulas on a case small enough to do by hand: 4 identical beats and an inverted fifth in one lead"""
    T, pos = 2000, [200, 500, 800, 1100, 1340]
    t = np.arange(T, dtype=np.float64)
    x = np.zeros((1, T))
    for k, p in enumerate(pos):
        x[0] += (-1.0 if k == 4 else 1.0) * np.exp(-0.5 * ((t - p) / 4.0) ** 2)
    lab, corr, rr = U.classify_record(x, pos)
    assert lab == [0, 0, 0, 0, 1] and np.isnan(rr[0]) and rr[1:4] == [1.0, 1.0, 1.0] and rr[4] == 240 / 300
    assert all(c > 0.999 for c in corr[:4]) and -1.0 < corr[4] < -0.8       # (the best shift is the least opposed: +-Sa)
    # three beats: two neighbours each, fewer than min_ref
    lab, corr, rr = U.classify_record(x, pos[:3])
    assert lab == [-1, -1, -1] and all(np.isnan(c) for c in corr) and all(np.isnan(r) for r in rr)
    # a constant record: the denominator is 0, corr = 0 < c0
    lab, corr, rr = U.classify_record(np.full((2, 500), 3.0), [50, 150, 250, 350])
    assert lab == [1, 1, 1, 1] and corr == [0.0] * 4


def test_make_records_with_rhythm():
    a = synth.make_records_with_rhythm(3, 2, 5000, seed=4, p_v=0.2, p_s=0.1)
    b = synth.make_records_with_rhythm(3, 2, 5000, seed=4, p_v=0.2, p_s=0.1)
    assert a[0].dtype == np.float32 and a[0].shape == (3, 2, 5000) and np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    assert not np.array_equal(a[0], synth.make_records_with_rhythm(3, 2, 5000, seed=5, p_v=0.2, p_s=0.1)[0])
    n_v = n_s = 0
    for seed in range(6):
        x, beats, labels = synth.make_records_with_rhythm(4, 3, 9000, seed=seed, p_v=0.3, p_s=0.2)
        for r in range(4):
            p, l = np.asarray(beats[r]), np.asarray(labels[r])
            assert len(p) == len(l) >= 15 and np.all(np.diff(p) > 0) and p[0] >= 0 and p[-1] < 9000
            assert set(l.tolist()) <= {0, 1, 2} and l[0] == 0
            assert not np.any((l[1:] != 0) & (l[:-1] != 0))         # never two ectopic beats in a row
            n_v, n_s = n_v + int((l == 1).sum()), n_s + int((l == 2).sum())
            rr = np.diff(p)
            base = np.median(rr[(l[1:] == 0) & (l[:-1] == 0)])
            assert np.all(rr[l[1:] != 0] < 0.85 * base)             # an ectopic beat comes early ...
            after = np.flatnonzero(l[:-1] != 0)
            assert np.all(rr[after] > 1.1 * base)                   # ... and a compensatory pause follows it
            inner = [(q, k) for q, k in zip(p, l) if 20 < q < 9000 - 20]
            assert all(abs(int(np.argmax(x[r, 0, q - 15:q + 16])) - 15) <= 1 for q, k in inner)      # lead 0: R upright
            assert all(abs(int(np.argmin(x[r, 1, q - 15:q + 16])) - 15) <= 1 for q, k in inner if k == 1)   # the odd lead: V upside down
    assert n_v >= 40 and n_s >= 20
    # p_s = 0 (the default) gives no S beat, p_v = 0 only normal ones
    assert all(2 not in l for l in synth.make_records_with_rhythm(4, 2, 9000, seed=1)[2])
    assert all(set(l) == {0} for l in synth.make_records_with_rhythm(4, 2, 9000, seed=1, p_v=0.0)[2])


def test_the_oracle_recovers_the_generator_labels_far_from_the_thresholds():
    """8 clean records of 30 s with p_v = 0.12, p_s = 0.08: among the classified beats whose extended window lies inside the
    record the oracle gives every generator label, and fewer than 1 % of the beats lie within the GPU comparison's tolerance of
    a threshold - what makes the exact label comparison on the GPU legitimate.  Here: 295 beats (242 N, 33 V, 20 S), none near;
    corr >= 0.994 for N and S, <= 0.25 for V; rr_ratio <= 0.76 for V and S, >= 0.90 for N."""
    R, leads, T = 8, 2, 10800
    x, beats, labels = synth.make_records_with_rhythm(R, leads, T, seed=11, p_v=0.12, p_s=0.08)
    g = U.geometry(360)
    ext = g["Wb"] + g["Sa"]
    total = near = 0
    seen = set()
    for r in range(R):
        lab, corr, rr = U.classify_record(x[r], beats[r])
        assert len(beats[r]) >= 9 and all(v >= 0 for v in lab)
        for i, (p, want) in enumerate(zip(beats[r], labels[r])):
            near += U.near_threshold(corr[i], rr[i], i, leads, 360)
            if ext <= p < T - ext:
                assert lab[i] == want, (r, i, p, want, lab[i], corr[i], rr[i])
                total += 1
                seen.add(want)
    n_all = sum(len(b) for b in beats)
    print(f"{total} inner beats of {n_all}, {near} near a threshold")
    assert seen == {0, 1, 2} and total >= 250
    assert near < 0.01 * n_all


def test_pool_planning_raising_calls_change_nothing():
    st = RhythmPoolState(2, 3, 360)
    a, b = st.open(), st.open()
    snap = lambda: (st.nb.copy(), st.done.copy(), st.beats.n.copy(), st.beats.turn.copy(), st.beats.is_open.copy(), list(st.beats.free))
    before = snap()
    for shapes, close in (({a: (2, 10), 2: (2, 10)}, ()), ({a: (1, 10)}, ()), ({a: (2,)}, ()), ({a: (2, 10)}, (7,)), ({}, ()),
                          ({a: (2, 1 << 30)}, ()), ({}, (b,)), ({True: (2, 10)}, ())):
        with pytest.raises(RalError):
            st.plan(shapes, close)
        assert all(np.array_equal(p, q) for p, q in zip(snap(), before))
    sids, btab = st.plan({a: (2, 4000), b: (2, 900)})
    assert sids == [a, b]
    with pytest.raises(RalError):
        st.table(btab, [1])
    with pytest.raises(RalError):
        st.table(btab, [1, -1])
    tab = st.table(btab, [5, 2])
    assert all(np.array_equal(p, q) for p, q in zip(snap(), before))        # planning changes nothing
    assert tab["m"].tolist() == [5, 2] and tab["ne"].tolist() == [0, 0] and tab["new_off"].tolist() == [0, 5]
    assert tab["turn"].tolist() == [0, 0] and tab["x_off"].tolist() == [0, 4000] and tab["T"].tolist() == [-1, -1]
    st.beats.commit(btab)
    st.commit(tab)
    assert st.nb[[a, b]].tolist() == [5, 2] and st.done[[a, b]].tolist() == [0, 0]
    # the ninth beat releases the first eight; a stream that ends releases what it has
    sids, btab = st.plan({a: (2, 3000)}, close=(b,))
    tab = st.table(btab, [4, 1])
    assert tab["nb"].tolist() == [5, 2] and tab["e0"].tolist() == [0, 0] and tab["ne"].tolist() == [9, 3]
    assert tab["out_off"].tolist() == [0, 9] and tab["turn"].tolist() == [1, 1] and tab["flags"].tolist() == [_lib.POOL_KEEP, 0]
    st.beats.commit(btab)
    st.commit(tab)
    assert st.nb[a] == st.done[a] == 9 and not st.beats.is_open[b]
    # from then on every beat comes out with the call that brings it, 20 at once as well
    for m in (0, 1, 20):
        sids, btab = st.plan({a: (2, 500)})
        tab = st.table(btab, [m])
        assert tab["e0"].tolist() == [st.nb[a]] and tab["ne"].tolist() == [m]
        st.beats.commit(btab)
        st.commit(tab)
    assert st.nb[a] == st.done[a] == 30
    # a reused slot starts again
    c = st.open()
    assert c == b and st.nb[c] == st.done[c] == 0
    with pytest.raises(RalError):
        RhythmPoolState(2, 0, 360)
    with pytest.raises(RalError):
        RhythmPoolState(52, 2, 360)                 # the detector's own limit


def test_header_exports_and_python_names_agree():
    hdr = open(os.path.join(ROOT, "include", "ralenet.h")).read()
    declared = {n for n in re.findall(r"\b(ral_[a-z_0-9]+)\s*\(", hdr) if n.startswith("ral_rhythm_")}
    want = {"ral_rhythm_records", "ral_rhythm_pool", "ral_rhythm_pool_scratch_bytes"}
    assert declared == want == {n for n in _lib.EXPORTS if n.startswith("ral_rhythm_")}
    L = _lib.lib()
    assert all(hasattr(L, n) for n in want)
    assert _lib.RHYTHM_ROW.itemsize == 80 and ctypes.sizeof(_lib.RhythmGeom) == 16
    assert (_lib.RHYTHM_K, _lib.RHYTHM_MIN_REF) == (8, 3) == (U.K, U.MIN_REF)
    assert "#define RAL_RHYTHM_K 8" in hdr and "#define RAL_RHYTHM_MIN_REF 3" in hdr
    for name in ("BeatClassifier", "BeatClasses", "BeatClassPool", "evaluate_rhythm", "rhythm_geometry", "rhythm_check"):
        assert hasattr(ecg_denoise_amd, name), name
    # the scratch query needs no device: bytes of the gathered windows, and the refusals
    geom = _lib.RhythmGeom(36, 3, 0.7, 0.8)
    assert L.ral_rhythm_pool_scratch_bytes(10, 2, geom) == 10 * 2 * 79 * 4
    assert L.ral_rhythm_pool_scratch_bytes(0, 2, geom) == 2 * 79 * 4
    for beats, leads, gm, rule in ((10, 0, geom, "leads"), (-1, 2, geom, "beats"), (10, 2, _lib.RhythmGeom(36, 28, 0.7, 0.8), "Sa <= 27"),
                                   (10, 2, _lib.RhythmGeom(2000, 3, 0.7, 0.8), "64 KB of LDS"),
                                   (10, 2, _lib.RhythmGeom(36, 3, float("nan"), 0.8), "finite")):
        assert L.ral_rhythm_pool_scratch_bytes(beats, leads, gm) == -1 and rule in L.ral_last_error().decode()
    # the host rule and the library's agree on what fits
    for fs in (360, 1000, 1450, 3000, 3400, 4000, 8000):
        g = rhythm_geometry(fs)
        fits = L.ral_rhythm_pool_scratch_bytes(1, 2, _lib.RhythmGeom(g["Wb"], g["Sa"], 0.7, 0.8)) > 0
        try:
            rhythm_check(fs, 2)
            assert fits, fs
        except RalError:
            assert not fits, fs


def test_pool_entry_point_checks_the_host_table_before_any_device_work():
    """`ral_rhythm_pool` walks the host table first: with pointers that are never dereferenced every broken rule is named, and a
    sound table reaches the scratch check - `_lib.RHYTHM_ROW` and `ral_rhythm_row` agree"""
    L = _lib.lib()
    st = RhythmPoolState(2, 3)
    a, b = st.open(), st.open()
    btab = st.plan({a: (2, 900), b: (2, 37)})[1]
    st.beats.commit(btab)
    st.commit(st.table(btab, [3, 0]))
    _, btab = st.plan({a: (2, 500)}, close=(b,))
    tab = st.table(btab, [7, 0])
    assert tab["ne"].tolist() == [10, 0]
    geom = _lib.RhythmGeom(36, 3, 0.7, 0.8)
    fake = 4096

    def call(t, x_total=500, new_total=7, out_total=10):
        rc = L.ral_rhythm_pool(fake, fake, x_total, t.ctypes.data, len(t), fake, 1, 3, 2, geom, st.beats.hist_len, fake, fake, fake,
                               new_total, fake, 0, fake, fake, fake, fake, out_total, None)
        return rc, L.ral_last_error().decode()

    def broken(field, row, value):
        t = tab.copy()
        t[field][row] = value
        return t

    for t, kw, rule in ((tab, {}, "scratch"), (broken("slot", 1, 3), {}, "0 <= slot < capacity"),
                        (broken("slot", 1, int(tab["slot"][0])), {}, "every slot at most once"),
                        (broken("x_off", 0, 1), {}, "the chunk inside the packed chunks"),
                        (broken("m", 0, 8), {}, "new beats inside the packed new beats"),
                        (tab, {"out_total": 9}, "results inside the packed results"),
                        (broken("e0", 0, 1), {}, "e0 \\+ ne = nb \\+ m"), (broken("turn", 0, 2), {}, "turn 0 or 1"),
                        (broken("T", 0, 5), {}, "T = n0 \\+ c"), (broken("c", 0, -1), {}, "0 <= c")):
        rc, msg = call(t, **kw)
        assert rc != 0 and msg.startswith("rhythm_pool: need ") and re.search(rule, msg), msg
    # beats that are not final yet: an open row may not give out fewer than K + 1
    t = broken("m", 0, 4)
    t["ne"][0] = 7
    rc, msg = call(t, new_total=4, out_total=7)
    assert rc != 0 and "beats that are final" in msg, msg
    t = tab.copy()
    t["nb"][0], t["e0"][0], t["ne"][0] = 12, 0, 19
    rc, msg = call(t, out_total=19)
    assert rc != 0 and "e0 = nb, or e0 = 0" in msg, msg
