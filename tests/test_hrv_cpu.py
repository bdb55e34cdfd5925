"""HRV without a device: the numpy oracle (tests/hrv_util.py) against scipy's Lomb-Scargle periodogram, against its golden file
and against a known modulation; the host side of `ecg_denoise_amd.hrv` (geometry, refusals, windows, `HrvPoolState`); the fp32
emulation of the kernel's arithmetic against the spectral tolerance; the generator."""
import os
from fractions import Fraction

import numpy as np
import pytest

import hrv_util as U


def _g(fs=360, **kw):
    from ecg_denoise_amd import hrv_geometry
    return hrv_geometry(fs, **kw)


def _series(fs, secs, amp, rr0=0.8, seed=0):
    """beats whose interval is rr0 + amp sin(2 pi 0.1 t) + amp / 2 sin(2 pi 0.25 t + 1), positions rounded to samples"""
    t, out = 0.3 + 0.01 * seed, []
    while t < secs:
        out.append(int(np.floor(t * fs + 0.5)))
        t += rr0 + amp * np.sin(2 * np.pi * 0.1 * t) + 0.5 * amp * np.sin(2 * np.pi * 0.25 * t + 1.0)
    return out


# ------------------------------------------------------------------------------------------------ the oracle
def test_oracle_equals_scipy_lombscargle():
    sig = pytest.importorskip("scipy.signal")
    from ecg_denoise_amd import synth
    beats, labels = synth.make_beats_with_hrv(2, 360 * 120, seed=5, p_v=0.05, p_s=0.05)
    g = _g(360, win_s=60, hop_s=30, min_nn=8)
    seen = 0
    for pos, lab in zip(beats, labels):
        for w0, w1 in U.windows(360 * 120, g):
            _, q, d, _ = U.nn_intervals(pos, lab, w0, w1, g)
            m = len(d)
            psd, S, _ = U.spectrum64(q, d, g)
            y = (np.asarray(d, dtype=np.float64) - sum(d) / m).astype(np.float32).astype(np.float64)
            ref = sig.lombscargle(np.asarray(q, dtype=np.float64) / 360.0, y, 2 * np.pi * g["freqs"]) * 2 / m
            P = psd * m * 360.0 ** 2 / 2                                  # the periodogram itself, in samples^2
            assert np.abs(P * 2 / m - ref).max() <= 1e-16 * (y * y).sum(), np.abs(P * 2 / m - ref).max() / (y * y).sum()
            seen += 1
    assert seen == 6


def test_oracle_equals_the_golden_file(golden_dir):
    z = np.load(os.path.join(golden_dir, "g11_hrv.npz"))
    g = _g(360, win_s=int(z["win_s"]), hop_s=int(z["hop_s"]), min_nn=int(z["min_nn"]))
    at = 0
    for r in range(3):
        n = int(z["n"][r])
        for o in U.oracle_record(z["pos"][r, :n], z["lab"][r, :n], int(z["T"]), g):
            assert o["counts"] == z["counts"][at].tolist()
            np.testing.assert_allclose(o["stats"], z["stats"][at], rtol=1e-12, atol=0, equal_nan=True)
            np.testing.assert_allclose(o["psd"], z["psd"][at], rtol=0, atol=1e-12 * z["S"][at], equal_nan=True)
            at += 1
    assert at == len(z["counts"]) == 30


@pytest.mark.parametrize("secs", [60, 300])
def test_a_known_modulation_gives_its_power_in_lf_and_hf(secs):
    """an RR series modulated with amplitude A at 0.1 Hz and A / 2 at 0.25 Hz: LF = A^2 / 2, HF = A^2 / 8, within 10 %"""
    A, fs = 0.04, 360
    g = _g(fs, win_s=secs, hop_s=secs)
    o = U.oracle(_series(fs, secs, A), None, 0, secs * fs, g)
    assert o["m"] >= 60 and o["counts"][1] == o["counts"][0] - 1
    assert abs(o["stats"][6] - A * A / 2) <= 0.10 * A * A / 2, o["stats"][6] / (A * A / 2)
    assert abs(o["stats"][7] - A * A / 8) <= 0.10 * A * A / 8, o["stats"][7] / (A * A / 8)
    assert abs(o["stats"][9] - 4.0) <= 0.8 and abs(o["stats"][1] - 75.0) < 1.0


def test_time_domain_by_hand():
    g = _g(360, win_s=30, hop_s=10, min_nn=8)
    pos = [100, 400, 700, 1030, 1330, 1630, 1631, 2000]       # intervals 300 300 330 300 300 1 369; the 1 is below lo_n = 108
    lab = [0, 0, 0, 0, 1, 0, 0, 0]                            # the V beat removes two intervals
    o = U.oracle(pos, lab, 0, 10800, g)
    assert o["counts"] == [8, 4, 2, 1]                        # NN: 300 300 330 and 369 (i = 1, 2, 3, 7); pairs (1,2), (2,3)
    d = np.array([300, 300, 330, 369]) / 360.0
    assert abs(o["stats"][0] - d.mean()) < 1e-15 and abs(o["stats"][2] - d.std(ddof=1)) < 1e-15
    assert abs(o["stats"][3] - np.sqrt((0 + 30 ** 2) / 2) / 360.0) < 1e-15 and o["stats"][4] == 0.5
    assert np.isnan(o["stats"][5:]).all()
    assert U.oracle(pos, None, 0, 10800, g)["counts"] == [8, 6, 4, 2]
    assert U.oracle(pos, lab, 400, 1631, g)["counts"] == [5, 2, 1, 1]


# ------------------------------------------------------------------------------------------------ geometry and refusals
def test_geometry_values():
    g = _g(360)
    assert (g["W"], g["H"], g["lo_n"], g["hi_n"], g["t50"], g["F"], g["min_nn"], g["max_m"]) == (108000, 21600, 108, 720, 18, 120, 16, 999)
    assert g["band"].tolist() == [0] * 11 + [1] * 33 + [2] * 75 + [-1] and g["band"].dtype == np.int32
    assert g["freqs"][0] == 1 / 300 and g["freqs"][11] == 12 / 300 and len(g["freqs"]) == 120
    g = _g(500)
    assert (g["W"], g["H"], g["lo_n"], g["hi_n"], g["t50"], g["F"], g["max_m"]) == (150000, 30000, 150, 1000, 25, 120, 999)
    g = _g(Fraction(725, 2))
    assert (g["W"], g["H"], g["lo_n"], g["hi_n"], g["t50"], g["F"], g["max_m"]) == (108750, 21750, 109, 725, 18, 120, 997)
    g = _g(Fraction(725, 2), win_s=30, hop_s=10, min_nn=8)                 # 10875 samples: f_k = (k + 1) 362.5 / 10875 = (k + 1) / 30
    assert (g["W"], g["H"], g["F"]) == (10875, 3625, 12) and g["band"].tolist() == [0, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, -1]
    g = _g(1024, win_s=1200)
    assert (g["W"], g["F"], g["max_m"], g["lo_n"]) == (1228800, 480, 3989, 308)
    g = _g(360, win_s=Fraction(1, 3), hop_s=0.5)                           # 120 and 180 samples; halves round up
    assert (g["W"], g["H"]) == (120, 180) and _g(3, win_s=0.5)["W"] == 2


def test_every_refusal_names_its_rule():
    from ecg_denoise_amd import HrvAnalyzer, HrvPoolState, RalError, hrv_check
    cases = [(dict(fs=1, win_s=1), "2 <= W < 2\\^31"), (dict(fs=1024, win_s=3000000), "2 <= W < 2\\^31"),
             (dict(fs=360, hop_s=0.001), "1 <= H"), (dict(fs=360, nn_range=(0, 2.0)), "1 <= lo_n <= hi_n"),
             (dict(fs=360, nn_range=(1.0, 0.5)), "1 <= lo_n <= hi_n"),
             (dict(fs=360, win_s=2, fmax=0.4), "1 <= F <= 4096"), (dict(fs=360, fmax=Fraction(1, 301)), "1 <= F <= 4096"),
             (dict(fs=360, fmax=20), "1 <= F <= 4096"),
             (dict(fs=1024, win_s=4000, nn_range=(1.0, 2.0)), "F \\* W < 2\\^31"),
             (dict(fs=1024, win_s=1200, nn_range=(0.25, 2.0)), "max_m = \\(W - 1\\) // lo_n <= 4096"),
             (dict(fs=360, min_nn=1), "2 <= min_nn")]
    for kw, rule in cases:
        with pytest.raises(RalError, match="need " + rule):
            hrv_check(_g(**kw))
        with pytest.raises(RalError, match="need " + rule):
            HrvAnalyzer(device="cpu", **kw)
    g = _g(1024, win_s=4000)                                   # the defaults at this length break F W < 2^31 and max_m as well
    assert g["F"] * g["W"] >= 2 ** 31 and g["max_m"] > 4096
    with pytest.raises(RalError):
        HrvPoolState(2, g)
    for bad in (dict(fs=0), dict(fs=360.5), dict(win_s="300"), dict(min_nn=16.0), dict(fmax=float("nan"))):
        with pytest.raises(RalError):
            _g(**bad)
    assert hrv_check(_g(360)) is not None and hrv_check(_g(1024, win_s=1200)) is not None


def test_windows_of_short_exact_and_nearly_two_window_records():
    from ecg_denoise_amd import RalError, hrv_windows
    g = _g(360, win_s=30, hop_s=10)
    W, H = g["W"], g["H"]
    assert hrv_windows(W - 1, g).tolist() == [[0, W - 1]] and hrv_windows(1, g).tolist() == [[0, 1]]
    assert hrv_windows(W, g).tolist() == [[0, W]]
    assert hrv_windows(W + H - 1, g).tolist() == [[0, W]]
    assert hrv_windows(W + H, g).tolist() == [[0, W], [H, W + H]]
    assert hrv_windows(W + 3 * H + 5, g).tolist() == [[k * H, k * H + W] for k in range(4)]
    for T in (1, W - 1, W, W + H - 1, W + H, 5 * W + 7):
        assert hrv_windows(T, g).tolist() == [list(w) for w in U.windows(T, g)]
    with pytest.raises(RalError):
        hrv_windows(0, g)


def test_analyse_checks_lists_on_the_host_before_any_device_work():
    from ecg_denoise_amd import HrvAnalyzer, RalError
    a = HrvAnalyzer(win_s=30, hop_s=10, device="cpu")
    for beats in ([[5, 5]], [[9, 3]], [[-1]], [[1, 1000]], []):
        with pytest.raises(RalError, match="strictly ascending|no record"):
            a.analyse(beats, 1000)
    with pytest.raises(RalError, match="one label per beat"):
        a.analyse([[1, 2, 3]], 1000, classes=[[0, 0]])
    with pytest.raises(RalError, match="T must be"):
        a.analyse([[1]], 0)
    with pytest.raises(RalError, match="runs on the GPU"):
        a.analyse([[1, 2, 3]], 1000)


# ------------------------------------------------------------------------------------------------ HrvPoolState
def _brute(pos, T, g):
    return [list(w) for w in U.windows(T, g)]


@pytest.mark.parametrize("seed", range(6))
def test_pool_state_emits_every_window_of_the_record_once_and_in_order(seed):
    """seeded random schedules of feeds and closes over three slots: per stream the windows emitted are the record's, in order,
    exactly once each; every window is emitted with all the beats that lie in it; calls that raise change nothing"""
    from ecg_denoise_amd import HrvPoolState, RalError
    rng = np.random.default_rng(100 + seed)
    g = _g(360, win_s=30, hop_s=10, min_nn=8)
    W, H = g["W"], g["H"]
    st = HrvPoolState(3, g)
    streams = []
    for s in range(5):
        T = int(rng.choice([W - 7, W, W + H - 1, 3 * W + 11, 5 * W + H // 2, 200]))
        n = int(rng.integers(0, T // 200 + 2))
        pos = np.sort(rng.choice(T, size=min(n, T), replace=False)).astype(np.int64) if rng.random() > 0.15 else np.zeros(0, dtype=np.int64)
        streams.append({"T": T, "pos": pos, "lab": rng.integers(-1, 3, len(pos)).astype(np.int32), "at": 0, "sid": None, "got": [],
                        "done": False})
    free = [2, 1, 0]
    while not all(s["done"] for s in streams):
        for s in streams:
            if s["sid"] is None and not s["done"] and free and rng.random() < 0.5:
                s["sid"] = free.pop()
                st.open(s["sid"])
        live = [s for s in streams if s["sid"] is not None and not s["done"]]
        if not live:
            continue
        snap = ([p.copy() for p in st.pos], [l.copy() for l in st.lab], st.emitted.copy(), st.last.copy(), st.is_open.copy())
        a = live[0]
        bad = [({7: ((), ())}, {}), ({a["sid"]: ((5, 6), (0,))}, {}), ({a["sid"]: ((9, 9), (0, 0))}, {}),
               ({}, {a["sid"]: int(a["pos"][a["at"] - 1]) if a["at"] else 0})]
        if a["at"]:
            bad.append(({a["sid"]: ((int(a["pos"][a["at"] - 1]),), (0,))}, {}))           # not beyond the last released beat
        for beats, close in bad:
            with pytest.raises(RalError):
                st.feed(beats, close)
        now = (st.pos, st.lab, st.emitted, st.last, st.is_open)
        assert all(np.array_equal(u, v) for x, y in zip(snap[:2], now[:2]) for u, v in zip(x, y))
        assert all(np.array_equal(u, v) for u, v in zip(snap[2:], now[2:]))
        beats, close = {}, {}
        for s in live:
            if rng.random() < 0.3:
                continue
            k = int(rng.integers(0, 12))
            hi = min(len(s["pos"]), s["at"] + k)
            if k:
                beats[s["sid"]] = (s["pos"][s["at"]:hi], s["lab"][s["at"]:hi])
            if hi == len(s["pos"]) and rng.random() < 0.5:
                close[s["sid"]] = s["T"]
            s["new_at"] = hi
        if not beats and not close:
            continue
        out = st.feed(beats, close)
        assert set(out) == set(beats) | set(close)
        for s in live:
            if s["sid"] not in out:
                continue
            w_first, win, pos, lab = out[s["sid"]]
            assert w_first == len(s["got"])
            for w0, w1 in win.tolist():
                inside = (s["pos"] >= w0) & (s["pos"] < w1)
                have = (pos >= w0) & (pos < w1)
                assert np.array_equal(pos[have], s["pos"][inside]) and np.array_equal(lab[have], s["lab"][inside])
                s["got"].append([w0, w1])
            if len(win) and s["sid"] not in close:                  # an open stream: final only behind a released beat
                assert s["pos"][s["new_at"] - 1] >= win[-1][0] + W
            s["at"] = s["new_at"]
            if s["sid"] in close:
                s["done"] = True
                free.append(s["sid"])
                assert not st.is_open[s["sid"]]
            else:                                                   # the state keeps the beats from the next origin onwards
                keep = s["pos"][:s["at"]]
                assert np.array_equal(st.pos[s["sid"]], keep[keep >= len(s["got"]) * H])
    for s in streams:
        assert s["got"] == _brute(s["pos"], s["T"], g), (s["T"], len(s["got"]))


# ------------------------------------------------------------------------------------------------ the spectral tolerance
@pytest.mark.parametrize("kind", ["short_360", "short_725_2", "ectopic", "long"])
def test_the_fp32_emulation_stays_within_the_spectral_tolerance(kind):
    """the kernel's arithmetic restated in numpy fp32 with sequential sums, on inputs of the kinds the device tests use: every
    bin within 4 (16 + m) 2^-24 S of the fp64 oracle, and the oracle's min(cc, ss) >= m / 4"""
    from ecg_denoise_amd import synth
    if kind == "long":
        fs, T = 1024, 1024 * 400
        g = _g(fs, win_s=400, hop_s=400)
        beats, labels = synth.make_beats_with_hrv(1, T, fs=fs, seed=3, lf=0.01, hf=0.005, bpm=(168.0, 172.0))
    else:
        fs = Fraction(725, 2) if kind == "short_725_2" else 360
        T = 120 * 360
        g = _g(fs, win_s=30, hop_s=10, min_nn=8)
        beats, labels = synth.make_beats_with_hrv(2, T, fs=float(fs), seed=4, p_v=0.06 if kind == "ectopic" else 0.0,
                                                  p_s=0.06 if kind == "ectopic" else 0.0)
    seen, worst = 0, 0.0
    for pos, lab in zip(beats, labels):
        for w0, w1 in U.windows(T, g)[::3]:
            _, q, d, _ = U.nn_intervals(pos, lab, w0, w1, g)
            if len(d) < g["min_nn"]:
                continue
            psd, S, den = U.spectrum64(q, d, g)
            m = len(d)
            assert den >= m / 4, (den, m)
            err = np.abs(U.emulate_psd(q, d, g).astype(np.float64) - psd).max()
            tol = 4 * (16 + m) * U.EPS * S
            assert err <= tol, (err / (U.EPS * S), m)
            worst, seen = max(worst, err / (U.EPS * S)), seen + 1
    assert seen >= (1 if kind == "long" else 6)
    assert worst <= 8, worst                       # (seen: 2.6) far inside the bound: the accumulation errors do not add up coherently


# ------------------------------------------------------------------------------------------------ the generator
def test_generator_properties():
    from ecg_denoise_amd import synth
    T = 360 * 300
    beats, labels = synth.make_beats_with_hrv(3, T, seed=9, lf=0.05, hf=0.02, p_v=0.05, p_s=0.05)
    again = synth.make_beats_with_hrv(3, T, seed=9, lf=0.05, hf=0.02, p_v=0.05, p_s=0.05)
    assert (beats, labels) == again and beats != synth.make_beats_with_hrv(3, T, seed=10, lf=0.05, hf=0.02, p_v=0.05, p_s=0.05)[0]
    for pos, lab in zip(beats, labels):
        assert len(pos) == len(lab) and all(isinstance(p, int) for p in pos) and set(lab) <= {0, 1, 2}
        assert pos[0] >= 0 and pos[-1] < T and all(b > a for a, b in zip(pos, pos[1:]))
        assert lab[0] == 0 and all(not (a and b) for a, b in zip(lab, lab[1:]))       # never two early beats in a row
        assert 200 <= len(pos) <= 520 and 1 in lab and 2 in lab
    # without ectopics the spectrum shows the modulation: LF = lf^2 / 2, HF = hf^2 / 2, within 10 %
    beats, labels = synth.make_beats_with_hrv(2, T, seed=9, lf=0.05, hf=0.02)
    g = _g(360)
    for pos, lab in zip(beats, labels):
        assert set(lab) == {0}
        o = U.oracle(pos, lab, 0, T, g)
        assert abs(o["stats"][6] - 0.05 ** 2 / 2) <= 0.10 * 0.05 ** 2 / 2 and abs(o["stats"][7] - 0.02 ** 2 / 2) <= 0.10 * 0.02 ** 2 / 2
    # other rates and heart rates
    b, _ = synth.make_beats_with_hrv(1, 1024 * 60, fs=1024, seed=1, lf=0.01, hf=0.005, bpm=(168.0, 172.0))
    assert 160 <= len(b[0]) <= 180
