"""Beat detection without a device: the bank, the geometry, the frontier, the synthetic truth lists, the ABI, the pool's
planning, and the guard that makes the exact comparisons of tests/test_gpu_beats.py legitimate."""
import os
import re

import numpy as np
import pytest

import beat_util as U
from ecg_denoise_amd import RalError, _lib, beat_bank, beat_frontier, beat_geometry, beat_latency, synth
from ecg_denoise_amd.beats import BeatPoolState, beat_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("fs", [360, 500, 250])
def test_bank_is_symmetric_and_has_no_dc_gain(fs):
    h = beat_bank(fs)
    g = beat_geometry(fs)
    assert h.dtype == np.float64 and h.shape == (2 * g["half"] + 1,)
    assert np.abs(h - h[::-1]).max() <= 1e-12 and abs(h.sum()) <= 1e-12
    assert np.array_equal(h, U.bank(fs))
    # a band-pass: the response at 16 Hz is near 1, at 1 Hz and at 60 Hz it is small
    k = np.arange(-g["half"], g["half"] + 1)
    gain = lambda f: abs(np.sum(h * np.exp(-2j * np.pi * f * k / fs)))
    assert 0.9 < gain(16) < 1.1 and gain(1) < 0.05 and gain(60) < 0.05
    with pytest.raises(RalError):
        beat_bank(fs, 24, 8)


def test_geometry_frontier_and_latency():
    assert beat_geometry(360) == {"half": 90, "Wi": 27, "Wt": 540, "Rf": 72, "Rw": 27}
    assert beat_geometry(500) == {"half": 125, "Wi": 38, "Wt": 750, "Rf": 100, "Rw": 38}       # 37.5 rounds up
    assert beat_geometry(250) == {"half": 63, "Wi": 19, "Wt": 375, "Rf": 50, "Rw": 19}         # 62.5 rounds up, 18.75 to 19
    for fs in (360, 500, 250, 128, 1000):
        g = beat_geometry(fs)
        assert g == U.geometry(fs)
        assert g["Rf"] <= g["Wt"] and 2 * g["Rw"] <= g["Rf"] and g["Rw"] <= g["Wt"] + g["Wi"]     # what the kernels rely on
        lag = g["Wt"] + g["Wi"] + g["half"]
        assert [beat_frontier(n, fs) for n in (0, lag, lag + 1, lag + 1000)] == [0, 0, 1, 1000]
        assert beat_latency(fs) == lag / fs
    assert beat_frontier(1000) == 343 and beat_frontier(657) == 0 and beat_frontier(658) == 1 and beat_latency() == 657 / 360
    with pytest.raises(RalError):
        beat_geometry(359.5)


def test_supported_pairs_of_rate_and_leads():
    for fs, leads in ((360, 1), (360, 12), (360, 51), (500, 12), (250, 2), (1000, 2)):
        assert beat_check(fs, leads) == beat_geometry(fs)
    for fs, leads in ((360, 52), (500, 40), (2000, 2), (360, 0)):
        with pytest.raises(RalError):
            beat_check(fs, leads)


def test_make_records_with_beats_equals_make_records():
    for R, leads, T, seed, block in ((3, 2, 1440, 5, 4096), (2, 1, 9000, 6, 4096), (2, 12, 700, 7, 256)):
        a = synth.make_records(R, leads, T, seed=seed, block=block)
        b, beats = synth.make_records_with_beats(R, leads, T, seed=seed, block=block)
        assert a.dtype == b.dtype and np.array_equal(a, b)
        assert len(beats) == R
        for r in range(R):
            p = np.asarray(beats[r])
            assert len(p) >= T // 500 and np.all(np.diff(p) > 0) and p[0] >= 0 and p[-1] < T
            inner = p[(p > 20) & (p < T - 20)]                   # lead 0 has its R wave's top there
            assert all(abs(int(np.argmax(a[r, 0, q - 15:q + 16])) - 15) <= 1 for q in inner)
    # what the docstring says of the truth list: seed 2023 at T = 4096 holds a pair closer than the refractory period
    _, beats = synth.make_records_with_beats(16, 2, 4096, seed=2023)
    assert min(np.diff(b).min() for b in beats) == 33 < beat_geometry(360)["Rf"]


def test_header_and_exports_agree_on_the_beat_entry_points():
    hdr = open(os.path.join(ROOT, "include", "ralenet.h")).read()
    declared = {n for n in re.findall(r"\b(ral_[a-z_0-9]+)\s*\(", hdr) if n.startswith("ral_beat_")}
    want = {"ral_beat_records", "ral_beat_records_scratch_bytes", "ral_beat_pool", "ral_beat_match"}
    assert declared == want == {n for n in _lib.EXPORTS if n.startswith("ral_beat_")}
    L = _lib.lib()
    assert all(hasattr(L, n) for n in want)
    assert _lib.BEAT_ROW.itemsize == 64 and __import__("ctypes").sizeof(_lib.BeatGeom) == 32
    # the shape checks of the scratch query need no device
    g = beat_geometry(360)
    geom = _lib.BeatGeom(g["half"], g["Wi"], g["Wt"], g["Rf"], g["Rw"], 0.35, 0.0, 0)
    assert L.ral_beat_records_scratch_bytes(4, 2, 1440, geom) >= 2 * 4 * 4 * 1440
    for R, leads, T, rule in ((65536, 2, 1440, "R <= 65535"), (4, 52, 1440, "64 KB of LDS"), (4, 2, 0, "1 <= T")):
        assert L.ral_beat_records_scratch_bytes(R, leads, T, geom) == -1 and rule in L.ral_last_error().decode()
    bad = _lib.BeatGeom(g["half"], g["Wi"], g["Wt"], g["Rf"], 40, 0.35, 0.0, 0)
    assert L.ral_beat_records_scratch_bytes(4, 2, 1440, bad) == -1 and "2 Rw <= Rf" in L.ral_last_error().decode()


def test_pool_planning_and_refusals():
    st = BeatPoolState(2, 3, 360)
    assert st.hist_len == 2 * 657
    a, b = st.open(), st.open()
    snap = lambda: (st.n.copy(), st.turn.copy(), st.is_open.copy(), list(st.free))
    before = snap()
    for shapes, close in (({a: (2, 10), 2: (2, 10)}, ()), ({a: (1, 10)}, ()), ({a: (2,)}, ()), ({a: (2, 10)}, (7,)), ({}, ()),
                          ({a: (2, 1 << 30)}, ()), ({}, (b,)), ({True: (2, 10)}, ())):
        with pytest.raises(RalError):
            st.plan(shapes, close)
        assert all(np.array_equal(p, q) for p, q in zip(snap(), before))
    sids, tab = st.plan({a: (2, 1000), b: (2, 40)}, close=(b,))
    assert sids == [a, b]
    assert tab["d0"].tolist() == [0, 0] and tab["d"].tolist() == [343, 40] and tab["T"].tolist() == [-1, 40]
    assert tab["cap"].tolist() == [343 // 73 + 1, 1] and tab["out_off"].tolist() == [0, 5] and tab["x_off"].tolist() == [0, 1000]
    assert st.span(tab) == 343 + 567
    assert all(np.array_equal(p, q) for p, q in zip(snap(), before))        # planning changes nothing
    st.commit(tab)
    assert st.n[a] == 1000 and st.turn[a] == 1 and not st.is_open[b] and st.free[-1] == b
    sids, tab = st.plan({a: (2, 1)})
    assert tab["d0"].tolist() == [343] and tab["d"].tolist() == [1] and tab["turn"].tolist() == [1]
    sids, tab = st.plan({a: (2, 0)})
    assert tab["d"].tolist() == [0] and tab["cap"].tolist() == [0] and st.span(tab) == 1
    sids, tab = st.plan({}, close=(a,))
    assert tab["d0"].tolist() == [343] and tab["d"].tolist() == [657] and tab["flags"].tolist() == [0]
    with pytest.raises(RalError):
        BeatPoolState(52, 3, 360)
    with pytest.raises(RalError):
        BeatPoolState(2, 0, 360)
    st1 = BeatPoolState(1, 1)
    st1.open()
    with pytest.raises(RalError, match="all 1 slots"):
        st1.open()


def test_matching_walk():
    assert U.match([], [], 54) == (0, 0, 0) and U.match([], [5, 900], 54) == (0, 2, 0) and U.match([100, 400], [], 54) == (0, 0, 2)
    assert U.match([100], [154], 54) == (1, 0, 0) and U.match([100], [155], 54) == (0, 1, 1)
    assert U.match([100, 200, 300], [40, 110, 150, 290, 1000], 54) == (3, 2, 0)


def test_the_oracle_decides_far_from_every_tie_on_the_shared_inputs():
    """What makes the exact comparison on the GPU legitimate: on each of the 30 records the oracle's threshold margin is at
    least 1e-2, the top of f leads its runner-up by at least 1e-5 (relative) and the refined peak keeps 2 samples from the
    window's edge - against fp32 rounding of about 1e-6 - and the same statements in fp32 give the same integers.
    Worst values here: 0.16, 2.3e-4, 13 samples."""
    worst = {"threshold": np.inf, "top": np.inf, "edge": np.inf}
    n = 0
    for name, x in U.inputs():
        for r, want in zip(x, U.expected()[name]):
            peaks, mg = U.detect(r, margins=True)
            assert peaks == want and len(peaks) >= 3
            assert peaks == U.detect(r, dtype=np.float32), name
            worst = {k: min(worst[k], mg[k]) for k in worst}
            n += 1
    print(f"worst margins over {n} records: {worst}")
    assert n == 30
    assert worst["threshold"] >= 1e-2 and worst["top"] >= 1e-5 and worst["edge"] >= 2


def test_pool_entry_point_checks_the_host_table_before_any_device_work():
    """`ral_beat_pool` walks the host table first: with pointers that are never dereferenced (the refusals come before any
    launch) every broken rule is named, and a sound table reaches the scratch check - `_lib.BEAT_ROW` and `ral_beat_row` agree"""
    from ecg_denoise_amd.beats import _Detector
    L = _lib.lib()
    st = BeatPoolState(2, 3)
    a, b = st.open(), st.open()
    st.commit(st.plan({a: (2, 900), b: (2, 37)})[1])
    _, tab = st.plan({a: (2, 500), b: (2, 50)})
    d = _Detector(360, 0.35, 0.0, (8, 24), 2, "cpu", "test")
    fake = 4096

    def call(t, hist_len=st.hist_len, ntaps=181):
        rc = L.ral_beat_pool(fake, fake, 550, t.ctypes.data, len(t), fake, 1, 3, 2, d.geom, fake, ntaps, hist_len, fake, 0, fake,
                             int(tab["cap"].sum()), fake, None)
        return rc, L.ral_last_error().decode()

    def broken(field, row, value):
        t = tab.copy()
        t[field][row] = value
        return t

    for t, kw, rule in ((tab, {}, "scratch"), (broken("d", 0, 501), {}, "decisions that are final"),
                        (broken("cap", 0, 2), {}, "cap >= ceil"), (broken("slot", 1, 0), {}, "every slot at most once"),
                        (broken("x_off", 1, 501), {}, "the chunk inside the packed chunks"),
                        (broken("n0", 0, 5900), {}, "inside the history"), (tab, {"hist_len": 10}, "hist_len >= 2"),
                        (tab, {"ntaps": 180}, "ntaps = 2 half")):
        rc, msg = call(t, **kw)
        assert rc != 0 and msg.startswith("beat_pool: need ") and rule in msg, msg
