"""The rhythm findings without a device: the geometry, the refusals of `arrhythmia_check` and of the C entry point, the numpy
oracle (tests/arrhythmia_util.py) on hand-written lists whose counts and flags are worked out here, `ArrhythmiaWindows.episodes`,
the AF generator, and the claim that makes the definition a detector of atrial fibrillation: at the true beats and labels, through
the committed delineation and P / ST oracles, irregular sinus rhythm with premature beats is IRREGULAR but never AF, and AF is."""
import ctypes as C
import functools
import hashlib
import json
from fractions import Fraction

import numpy as np
import pytest
import torch

import arrhythmia_util as A
import pst_util as P

from ecg_denoise_amd import _lib

NAN = float("nan")


# ---------------------------------------------------------------------------------------------------------------- geometry
@pytest.mark.parametrize("fs,want", [
    (360, dict(W=10800, H=3600, lo_n=108, hi_n=720, bin=9, G=24, lock_n=7, prmax=144, pause_n=720, min_m=12, vrun_min=3, max_m=99)),
    # 500 Hz: fs / 40 = 12.5 rounds up to 13; max_m = 14999 // 150
    (500, dict(W=15000, H=5000, lo_n=150, hi_n=1000, bin=13, G=24, lock_n=10, prmax=200, pause_n=1000, min_m=12, vrun_min=3, max_m=99)),
    # 362.5 Hz: ceil(108.75) = 109, floor(725) = 725, 9.0625 -> 9, 7.25 -> 7, round(145) = 145; max_m = 10874 // 109
    (Fraction(725, 2), dict(W=10875, H=3625, lo_n=109, hi_n=725, bin=9, G=24, lock_n=7, prmax=145, pause_n=725, min_m=12,
                            vrun_min=3, max_m=99)),
])
def test_geometry(fs, want):
    from ecg_denoise_amd import arrhythmia_check, arrhythmia_geometry
    g = arrhythmia_check(arrhythmia_geometry(fs))
    assert {k: g[k] for k in want} == want
    assert {k: A.geometry(fs)[k] for k in want} == want
    assert (g["n0"], g["c0"], g["pl0"], g["tachy"], g["brady"]) == (0.10, 0.6, 0.5, 100.0, 50.0) and g["fs"] == Fraction(fs)
    small = arrhythmia_geometry(fs, win_s=8, hop_s=4, pause_s=1.5, min_m=5)
    assert (small["W"], small["H"], small["pause_n"], small["min_m"]) == (8 * Fraction(fs), 4 * Fraction(fs),
                                                                        (Fraction(3, 2) * Fraction(fs)).__floor__(), 5)
    assert arrhythmia_geometry(20)["bin"] == 1                       # fs / 40 = 0.5 rounds to 1, and max(1, .) holds below that
    assert arrhythmia_geometry(10)["bin"] == 1


@pytest.mark.parametrize("change,rule", [
    (dict(W=1), "2 <= W < 2^31"), (dict(W=2 ** 31), "2 <= W < 2^31"), (dict(H=0), "1 <= H"), (dict(lo_n=0), "1 <= lo_n <= hi_n"),
    (dict(lo_n=721), "1 <= lo_n <= hi_n"), (dict(max_m=4097), "max_m = (W - 1) // lo_n <= 4096"), (dict(bin=0), "1 <= bin"),
    (dict(G=0), "1 <= G <= 64"), (dict(G=65), "1 <= G <= 64"), (dict(lock_n=-1), "0 <= lock_n"), (dict(prmax=0), "1 <= prmax <= 8192"),
    (dict(prmax=8193), "1 <= prmax <= 8192"), (dict(pause_n=0), "1 <= pause_n"), (dict(min_m=1), "2 <= min_m"),
    (dict(vrun_min=0), "1 <= vrun_min"), (dict(n0=NAN), "finite limits"), (dict(c0=float("inf")), "finite limits"),
    (dict(pl0=-float("inf")), "finite limits"), (dict(tachy=float("inf")), "finite limits"), (dict(brady=NAN), "finite limits"),
])
def test_check_names_the_broken_rule(change, rule):
    from ecg_denoise_amd import RalError, arrhythmia_check, arrhythmia_geometry
    g = dict(arrhythmia_geometry(360), **change)
    with pytest.raises(RalError) as e:
        arrhythmia_check(g)
    assert f"need {rule}" in str(e.value) and str(e.value).startswith("arrhythmia: this geometry is not supported")


def test_constructor_refuses_before_touching_the_library(monkeypatch):
    from ecg_denoise_amd import ArrhythmiaAnalyzer, RalError

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_library)
    with pytest.raises(RalError, match="need 1 <= pause_n"):
        ArrhythmiaAnalyzer(pause_s=0.001)
    with pytest.raises(RalError, match="need 2 <= min_m"):
        ArrhythmiaAnalyzer(min_m=1)
    with pytest.raises(RalError, match=r"need max_m = \(W - 1\) // lo_n <= 4096"):
        ArrhythmiaAnalyzer(win_s=1300)
    with pytest.raises(RalError, match="need 1 <= prmax <= 8192"):
        ArrhythmiaAnalyzer(fs=25000)
    with pytest.raises(RalError, match="min_m must be an int"):
        ArrhythmiaAnalyzer(min_m=12.0)
    with pytest.raises(RalError, match="n0 must be a number"):
        ArrhythmiaAnalyzer(n0="0.1")
    ana = ArrhythmiaAnalyzer()
    for T in (0, 2 ** 31, True, 10.0):
        with pytest.raises(RalError, match=r"ArrhythmiaAnalyzer.analyse: T must be in \[1, 2\^31\)"):
            ana.analyse([[5]], T)


# ------------------------------------------------------------------------------------------------- the C entry point's refusals
_OPERANDS = ("peaks", "label", "count", "on", "ppeak", "table", "table_dev", "geom", "counts", "stats", "flags")
_GEOM = dict(W=10800, lo_n=108, hi_n=720, bin=9, G=24, lock_n=7, prmax=144, pause_n=720, min_m=12, vrun_min=3, n0=0.1, c0=0.6, pl0=0.5,
             tachy=100.0, brady=50.0, pad_=0, fs=360.0)
_ROW_OK = (0, 10800, 0)
_REFUSALS = (
    [({p: None}, f"a non-null {p}") for p in ("peaks", "count", "table", "table_dev", "geom", "counts", "stats", "flags")]
    + [(dict(on=None), "on and ppeak together or neither (on is null)"), (dict(ppeak=None), "on and ppeak together or neither (ppeak is null)"),
       (dict(R=0), "1 <= R <= 65535"), (dict(R=65536), "1 <= R <= 65535"), (dict(cap=0), "1 <= cap < 2^31"),
       (dict(cap=2 ** 31), "1 <= cap < 2^31"), (dict(W=1), "2 <= W < 2^31"), (dict(W=-5), "2 <= W < 2^31"),
       (dict(lo_n=0), "1 <= lo_n <= hi_n"), (dict(hi_n=107), "1 <= lo_n <= hi_n"), (dict(lo_n=2, hi_n=2), "max_m = (W - 1) // lo_n <= 4096"),
       (dict(bin=0), "1 <= bin"), (dict(G=0), "1 <= G <= 64"), (dict(G=65), "1 <= G <= 64"), (dict(lock_n=-1), "0 <= lock_n"),
       (dict(prmax=0), "1 <= prmax <= 8192"), (dict(prmax=8193), "1 <= prmax <= 8192"), (dict(pause_n=0), "1 <= pause_n"),
       (dict(min_m=1), "2 <= min_m"), (dict(vrun_min=0), "1 <= vrun_min"), (dict(n0=NAN), "finite limits"),
       (dict(c0=float("inf")), "finite limits"), (dict(pl0=NAN), "finite limits"), (dict(tachy=-float("inf")), "finite limits"),
       (dict(brady=NAN), "finite limits"), (dict(fs=0.0), "a finite fs > 0"), (dict(rows=-1), "0 <= rows < 2^31"),
       (dict(row=(0, 10800, 2)), "0 <= rec < R in row 1"), (dict(row=(0, 10800, -1)), "0 <= rec < R in row 1"),
       (dict(row=(-1, 100, 0)), "0 <= w0 < w1 <= w0 + W in row 1"), (dict(row=(100, 100, 0)), "0 <= w0 < w1 <= w0 + W in row 1"),
       (dict(row=(0, 10801, 0)), "0 <= w0 < w1 <= w0 + W in row 1")])


def _call(**kw):
    """ral_arrhythmia_windows on host memory, two records and two table rows, with `kw` changed -> (rc, message)"""
    host = np.zeros(64, np.int32)
    ptr = {p: host.ctypes.data_as(C.c_void_p) for p in _OPERANDS}
    a = dict(R=2, cap=8, rows=2, upload=1)
    geom = dict(_GEOM)
    tab = np.zeros(2, dtype=_lib.HRV_ROW)
    tab["w0"], tab["w1"], tab["rec"] = (_ROW_OK[0],) * 2, (_ROW_OK[1],) * 2, (_ROW_OK[2],) * 2
    ptr["table"] = C.c_void_p(tab.ctypes.data)
    for k, v in kw.items():
        if k in ptr:
            ptr[k] = C.c_void_p(0)
        elif k in geom:
            geom[k] = v
        elif k == "row":
            tab["w0"][1], tab["w1"][1], tab["rec"][1] = v
        else:
            a[k] = v
    g = _lib.ArrhythmiaGeom(*geom.values())
    L = _lib.lib()
    L.ral_param_floats(C.byref(_lib.make_config("full", 2, 512, 0, 1)))     # leaves another message behind
    rc = L.ral_arrhythmia_windows(ptr["peaks"], ptr["label"], ptr["count"], ptr["on"], ptr["ppeak"], a["R"], a["cap"], ptr["table"],
                                  a["rows"], ptr["table_dev"], a["upload"], None if "geom" in kw else C.byref(g), ptr["counts"],
                                  ptr["stats"], ptr["flags"], C.c_void_p(0))
    return rc, L.ral_last_error().decode()


@pytest.mark.parametrize("kw,msg", _REFUSALS, ids=["-".join(f"{k}={v}" for k, v in kw.items()) for kw, _ in _REFUSALS])
def test_entry_point_refuses_bad_arguments_before_any_hip_call(kw, msg):
    """every refusal comes with "ral_arrhythmia_windows: need <the one rule that is broken>" and before any HIP call: this runs
    without a device (the operand pointers are host memory that a launch would fault on)"""
    rc, err = _call(**kw)
    assert rc != 0 and err.startswith(f"ral_arrhythmia_windows: need {msg}"), (rc, err)


# ------------------------------------------------------------------------------------------- the oracle on hand-written lists
G8 = A.geometry(360, win_s=8, hop_s=4)             # W = 2880, H = 1440; bin = 9, lock_n = 7, prmax = 144, pause_n = 720, min_m = 12


def _one(pos, T, lab=None, on=None, ppeak=None, g=G8):
    c, s, f, ix = A.analyse([pos], T, g, None if lab is None else [lab], None if on is None else [on], None if ppeak is None else [ppeak])
    return [tuple(r) for r in c.tolist()], s, f.tolist()


def _f32(v):
    return np.float32(np.float64(v))


def test_oracle_on_a_bigeminal_list():
    """16 beats whose intervals alternate 120 and 220 samples: every difference is +-100, the Lorenz points fall into the two
    cells (11, -11) and (-11, 11) - (200 + 9) // 18 = 11, (-200 + 9) // 18 = -11 - so the rhythm is as variable as AF by RMSSD
    (0.6) and not IRREGULAR by the grid (2 / 13 cells); 129.6 bpm is TACHY"""
    pos = [100]
    for i in range(15):
        pos.append(pos[-1] + (120 if i % 2 == 0 else 220))
    assert pos[-1] == 2600
    c, s, f = _one(pos, 2880)
    assert c == [(16, 15, 14, 13, 2, 0, 0, 0, 0, -1, 0, 0, 0)] and f == [A.TACHY]
    want = [_f32(2500 / (15 * 360.0)), _f32(60.0 * 15 * 360.0 / 2500), _f32(np.sqrt(140000 / 14) / (2500 / 15)), _f32(2 / 13), np.float32(NAN)]
    assert A.same_bits(s[0], want) and abs(float(s[0][2]) - 0.6) < 1e-6
    # the P input: PR 60 at ten beats, 70 at three, 30 at three -> lower median sorted[7] = 60, locked |pr - 60| <= 7: ten
    pr = [60] * 10 + [70] * 3 + [30] * 3
    on = [p - 20 for p in pos]
    c, s, f = _one(pos, 2880, on=on, ppeak=[o - v for o, v in zip(on, pr)])
    assert c == [(16, 15, 14, 13, 2, 0, 16, 16, 10, 60, 0, 0, 0)] and f == [A.TACHY] and s[0][4] == np.float32(0.625)
    # a PR of 0 or beyond prmax is measured and not found; on < 0 is not measured; a V beat is not measured
    ppeak = [o - v for o, v in zip(on, pr)]
    ppeak[0], ppeak[1], on[2], ppeak[3] = on[0], on[1] - 145, -1, -1
    lab = [0] * 16
    lab[4] = 1
    c, s, f = _one(pos, 2880, lab=lab, on=on, ppeak=ppeak)
    # V at index 4 takes intervals 4 and 5 out: m = 13; differences need i - 1 and i: 4, 5, 6 go: k = 11; points lose 4 .. 7: k2 = 9
    # found: five times 60, three times 70, three times 30 -> sorted[5] = 60, five locked
    assert c == [(16, 13, 11, 9, 2, 0, 14, 11, 5, 60, 0, 1, 1)], c
    assert s[0][4] == _f32(5 / 14)


def test_oracle_on_a_v_run_that_straddles_a_window_edge_and_on_pauses():
    """T = 4320: windows [0, 2880) and [1440, 4320).  V beats at 2700, 2800 and 2900: the first window holds two of them, no VRUN;
    the second all three.  Intervals above 720 samples are pauses whatever the labels."""
    pos = [200, 1000, 1800, 2700, 2800, 2900, 3500, 4000]
    lab = [0, 0, 0, 1, 1, 1, 0, 0]
    c, s, f = _one(pos, 4320, lab=lab)
    assert c[0] == (5, 0, 0, 0, 0, 0, 0, 0, 0, -1, 3, 2, 2) and f[0] == A.PAUSE and np.isnan(s[0]).all()
    # second window: members 1800 .. 4000; 1800 -> 2700 is a pause; the only accepted interval is 3500 -> 4000: 43.2 bpm
    assert c[1] == (6, 1, 0, 0, 0, 0, 0, 0, 0, -1, 1, 3, 3) and f[1] == A.PAUSE | A.VRUN | A.BRADY
    assert A.same_bits(s[1], [_f32(500 / 360.0), _f32(60.0 * 360.0 / 500), NAN, NAN, NAN])
    c, s, f = _one([100, 400, 1200], 2880)                                       # one pause
    assert c == [(3, 1, 0, 0, 0, 0, 0, 0, 0, -1, 1, 0, 0)] and f == [A.PAUSE] and s[0][1] == _f32(60.0 * 360.0 / 300)


def test_oracle_on_a_short_and_on_an_empty_record():
    c, s, f = _one([100, 500, 900], 1000)                                        # T < W: the single window [0, T)
    assert A.windows(1000, G8) == [(0, 1000)]
    assert c == [(3, 2, 1, 0, 0, 0, 0, 0, 0, -1, 0, 0, 0)] and f == [0]
    assert A.same_bits(s[0], [_f32(800 / 720.0), _f32(60.0 * 2 * 360.0 / 800), np.float32(0), NAN, NAN])
    c, s, f = _one([], 6000, on=[], ppeak=[])
    assert c == [(0, 0, 0, 0, 0, 0, 0, 0, 0, -1, 0, 0, 0)] * 3 and f == [0, 0, 0] and np.isnan(s).all()
    assert A.windows(6000, G8) == [(0, 2880), (1440, 4320), (2880, 5760)]
    assert [A.cell(D, G8) for D in (-5, -4, 4, 5, 13, 14, 10 ** 6, -10 ** 6)] == [-1, 0, 0, 1, 1, 2, 24, -24]


def test_irregular_needs_the_grid_and_af_needs_missing_pr_lock():
    """a list with 14 distinct differences in distinct cells is IRREGULAR; with a locked PR it is not AF, with a scattered PR or
    without P input it is"""
    d = [200, 260, 180, 330, 240, 400, 210, 300, 150, 280, 390, 170, 310, 230, 360]
    pos = [int(v) for v in np.cumsum([100] + d)]
    assert pos[-1] < 4320
    g = A.geometry(360, win_s=12, hop_s=12)
    c, s, f = _one(pos, 4320, g=g)
    assert c[0][:6] == (16, 15, 14, 13, 13, 0) and f == [A.IRREGULAR | A.AF]
    on = [p - 20 for p in pos]
    c, s, f = _one(pos, 4320, on=on, ppeak=[o - 60 for o in on], g=g)
    assert c[0][6:10] == (16, 16, 16, 60) and f == [A.IRREGULAR]
    c, s, f = _one(pos, 4320, on=on, ppeak=[o - 20 - 8 * i for i, o in enumerate(on)], g=g)        # PR 20, 28, ... 140
    assert c[0][6:10] == (16, 16, 1, 76) and f == [A.IRREGULAR | A.AF]


# --------------------------------------------------------------------------------------------------------------- episodes
def test_episodes_merge_runs_of_flagged_windows():
    from ecg_denoise_amd import ArrhythmiaWindows, arrhythmia_geometry
    g = arrhythmia_geometry(360)
    win = np.array([[w * 3600, w * 3600 + 10800] for w in range(7)], dtype=np.int64)
    flags = torch.tensor([1, 33, 0, 2, 35, 33, 1,          # record 0: runs 0 - 1 and 4 - 6
                          0, 0, 0, 0, 0, 0, 0,             # record 1: none
                          8, 8, 1, 0, 1, 0, 16], dtype=torch.int32)
    index = np.stack([np.repeat(np.arange(3), 7), np.tile(np.arange(7), 3)], axis=1)
    rh = ArrhythmiaWindows(torch.zeros(21, 13, dtype=torch.int32), torch.zeros(21, 5), flags, index, np.tile(win, (3, 1)), g)
    assert rh.episodes() == rh.episodes("af") == [[(0, 14400), (14400, 32400)], [], [(7200, 18000), (14400, 25200)]]
    assert rh.episodes("pause") == [[], [], [(0, 14400)]]
    assert rh.episodes("vrun") == [[], [], [(21600, 32400)]]
    assert rh.episodes("irregular") == [[(3600, 14400), (14400, 28800)], [], []]
    assert rh.af.tolist() == [bool(v & 1) for v in flags.tolist()] and rh.vrun.dtype == torch.bool
    assert rh.vrun_len.shape == rh.nrmssd.shape == rh.p_locked.shape == (21,)
    assert rh.tolist()[8]["record"] == 1 and rh.tolist()[8]["w0"] == 3600
    with pytest.raises(_lib.RalError, match="no finding named 'flutter'"):
        rh.episodes("flutter")


def test_af_truth_and_scores():
    from ecg_denoise_amd import af_scores, af_truth
    win = np.array([[w * 3600, w * 3600 + 10800] for w in range(7)], dtype=np.int64)
    index = np.stack([np.zeros(7, dtype=np.int64), np.arange(7)], axis=1)
    positive, scored = af_truth(win, index, [[(3600, 21600)]])                   # windows 1, 2 and 3 lie inside, 6 lies apart
    assert positive.tolist() == [False, True, True, True, False, False, False]
    assert scored.tolist() == [False, True, True, True, False, False, True]
    sc = af_scores([True, True, False, True, True, True, True], positive, scored)
    assert sc == dict(tp=2, fp=1, fn=1, tn=0, sensitivity=2 / 3, specificity=0.0)
    none = af_scores([False] * 7, [False] * 7, [False] * 7)
    assert np.isnan(none["sensitivity"]) and np.isnan(none["specificity"])


# --------------------------------------------------------------------------------------------------------------- generator
def _digest(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update((np.round(np.ascontiguousarray(p, dtype=np.float64), 5) + 0.0).tobytes() if isinstance(p, np.ndarray)
                 else json.dumps(p).encode())
    return h.hexdigest()[:16]


DIGESTS = {"make_records": "eb98fcf6302d6fcc", "make_records_with_beats": "ff68be1df0a8787d",
           "make_records_with_rhythm": "57e53cb4da21a128", "make_beats_with_hrv": "c6a568bc45c0819d",
           "make_noise_record": "034b544e0d25f995", "make_dataset": "45e87ede9d827bb5"}


def test_the_other_generators_keep_their_draws():
    """digests (the samples rounded to 1e-5) taken before `make_records_with_af` existed"""
    from ecg_denoise_amd import synth as s
    s.make_records_with_af(1, 1, 2000, seed=7)
    x, b = s.make_records_with_beats(2, 2, 5000, seed=7, block=2048)
    y, bb, ll = s.make_records_with_rhythm(2, 2, 3000, seed=7, p_v=0.12, p_s=0.2)
    hb, hl = s.make_beats_with_hrv(2, 40000, seed=7, p_v=0.05, p_s=0.1)
    n, c = s.make_dataset(n=3, L=128, seed=7)
    got = {"make_records": _digest(s.make_records(2, 2, 5000, seed=7, block=2048)), "make_records_with_beats": _digest(x, b),
           "make_records_with_rhythm": _digest(y, bb, ll), "make_beats_with_hrv": _digest(hb, hl),
           "make_noise_record": _digest(s.make_noise_record("emb", 2, 2000, seed=7)), "make_dataset": _digest(n, c)}
    assert got == DIGESTS


T90, SEED = 90 * 360, 2023


@functools.lru_cache(maxsize=None)
def _af_records():
    from ecg_denoise_amd import synth
    return synth.make_records_with_af(8, 2, T90, seed=SEED)


def test_generator_is_deterministic_and_its_episodes_lie_inside_the_record():
    from ecg_denoise_amd import synth
    x, beats, labels, eps = _af_records()
    x2, beats2, labels2, eps2 = synth.make_records_with_af(8, 2, T90, seed=SEED)
    assert x.dtype == np.float32 and x.shape == (8, 2, T90) and np.array_equal(x, x2) and (beats, labels, eps) == (beats2, labels2, eps2)
    x3, beats3, _, _ = synth.make_records_with_af(8, 2, T90, seed=SEED + 1)
    assert beats3 != beats
    for r in range(8):
        p = np.array(beats[r])
        assert p[0] >= 0 and p[-1] < T90 and (np.diff(p) >= 108).all() and labels[r] == [0] * len(p)
        (s, e), = eps[r]
        assert 0 <= s < e <= T90 and s in beats[r] and (e in beats[r] or e == T90)
        assert 0.3 - 0.02 <= (e - s) / T90 <= 0.6 + 0.05, (r, s, e)
        inside, outside = np.diff(p[(p >= s) & (p < e)]), np.diff(p[p < s])
        # the intervals inside the episode scatter by cv >= 0.15 (clipped at 0.3 s), the sinus intervals by 3 %
        assert inside.std() / inside.mean() > 0.09 and outside.std() / outside.mean() < 0.06, (r, inside.std() / inside.mean())


def test_af_beats_carry_no_p_wave_beyond_the_f_wave():
    """in front of a sinus beat lead 0 rises to the P wave, at least 0.8 * 0.12 mV; in front of an AF beat that follows a long
    interval (so that the previous T wave is over) nothing exceeds the f wave's amplitude, f_amp <= 0.06 mV"""
    x, beats, labels, eps = _af_records()
    seen_af = seen_sinus = 0
    for r in range(8):
        (s, e), = eps[r]
        p = beats[r]
        for i in range(1, len(p)):
            if p[i] - p[i - 1] < 270 or p[i] < 120:
                continue
            peak = np.abs(x[r, 0, p[i] - 100:p[i] - 50]).max()                   # 0.28 .. 0.14 s in front of the R peak
            if s <= p[i] < e:
                seen_af += 1
                assert peak <= 0.06 + 0.005, (r, i, peak)
            elif p[i] < s - 400 or p[i] > e + 400:
                seen_sinus += 1
                assert peak >= 0.8 * 0.12 * 0.9, (r, i, peak)
    assert seen_af >= 40 and seen_sinus >= 100, (seen_af, seen_sinus)


# -------------------------------------------------------------------------------------------------------------- separation
def _chain(x, beats, labels, T):
    """the committed delineation and P / ST oracles at the true beats, then this oracle at the true labels"""
    g = A.geometry(360)
    on, ppeak = [], []
    for r in range(len(beats)):
        res = P.delineate_and_measure(x[r], beats[r])
        on.append(res[0]), ppeak.append(res[3])
    return A.analyse(beats, T, g, labels, on, ppeak), A.windows(T, g)


@functools.lru_cache(maxsize=None)
def _af_chain():
    x, beats, labels, eps = _af_records()
    return _chain(x, beats, labels, T90)


@pytest.mark.parametrize("p_v,p_s,irregular", [(0.0, 0.0, None), (0.12, 0.0, None), (0.0, 0.3, True), (0.0, 1.0, True)])
def test_no_window_of_sinus_rhythm_with_ectopy_is_af(p_v, p_s, irregular):
    """8 records of 90 s of `make_records_with_rhythm`: no window gets the AF bit; with premature beats of normal shape every
    window is IRREGULAR, so it is the P evidence that keeps AF away"""
    from ecg_denoise_amd import synth
    x, beats, labels = synth.make_records_with_rhythm(8, 2, T90, seed=SEED, p_v=p_v, p_s=p_s)
    (c, s, f, ix), wins = _chain(x, beats, labels, T90)
    assert len(f) == 8 * 7
    print(f"p_v={p_v} p_s={p_s}: AF {int(((f & A.AF) != 0).sum())}, IRREGULAR {int(((f & A.IRREGULAR) != 0).sum())} of {len(f)}; "
          f"p_share {np.nanmin(s[:, 4]):.3f} .. {np.nanmax(s[:, 4]):.3f}")
    assert not (f & A.AF).any()
    if irregular:
        assert ((f & A.IRREGULAR) != 0).all()


def test_af_windows_are_flagged_and_windows_outside_the_episode_are_not():
    """8 records of 90 s of `make_records_with_af`: no window disjoint from the episode gets the AF bit, and at least 80 % of the
    windows wholly inside it do (a floor; this seed gives 9 of 9)"""
    x, beats, labels, eps = _af_records()
    (c, s, f, ix), wins = _af_chain()
    inside = apart = inside_af = 0
    for (r, w), flags in zip(ix.tolist(), f.tolist()):
        (w0, w1), (s0, e0) = wins[w], eps[r][0]
        if s0 <= w0 and w1 <= e0:
            inside += 1
            inside_af += bool(flags & A.AF)
        elif w1 <= s0 or e0 <= w0:
            apart += 1
            assert not flags & A.AF, (r, w, flags)
    print(f"AF windows flagged: {inside_af} of {inside} inside an episode; {apart} windows apart, none flagged")
    assert inside >= 8 and apart >= 4
    assert inside_af >= 0.8 * inside, (inside_af, inside)
