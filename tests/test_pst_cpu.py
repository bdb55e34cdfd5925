"""The P-wave and ST-level measurement without a device: the geometry, the host-side refusals, and what the numpy oracle
(tests/pst_util.py) says about the synthetic rhythm records - the properties that make the definition a measurement of the P
wave and of the ST level, checked on the oracle alone."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

import delineate_util as U
import pst_util as P

T, FS = 3600, 360
SEED = 24          # (checked with the oracle alone: every claim below holds for these four records)


@pytest.mark.parametrize("fs,want", [
    (360, dict(m2=6, g=7, Wp=108, j=22)),            # 7.2 -> 7, 21.6 -> 22
    (500, dict(m2=8, g=10, Wp=150, j=30)),           # 8.33 -> 8
    (250, dict(m2=4, g=5, Wp=75, j=15)),             # 4.17 -> 4
    (1000, dict(m2=17, g=20, Wp=300, j=60)),         # 16.67 -> 17
])
def test_geometry(fs, want):
    from ecg_denoise_amd import delineate_geometry, pst_check, pst_geometry
    assert pst_geometry(fs) == want == P.geometry(fs)
    assert pst_geometry(Fraction(fs)) == want
    assert pst_check(fs, 12) == want
    d = delineate_geometry(fs)                       # the lengths it shares with the delineator are the delineator's
    assert (want["m2"], want["g"], want["j"]) == (d["m2"], d["g"], d["gt"])
    assert pst_geometry(Fraction(725, 2)) == dict(m2=6, g=7, Wp=109, j=22)          # 362.5 Hz: 108.75 -> 109, 21.75 -> 22
    assert pst_geometry(125)["Wp"] == 38                                             # 37.5 rounds up


def test_check_refuses_an_oversized_rate_before_touching_the_library(monkeypatch):
    from ecg_denoise_amd import PStMeasurer, RalError, _lib, pst_check

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_library)
    with pytest.raises(RalError, match="fs=60000 is not supported.*18001 and 20001 samples.*64 KB of LDS"):
        pst_check(60000, 2)
    for leads in (0, 65536, True, 2.0):
        with pytest.raises(RalError, match="leads"):
            pst_check(360, leads)
    assert pst_check(25000, 2)["Wp"] == 7500                     # 7 501 + 8 335 floats fit
    with pytest.raises(RalError, match="not supported"):          # ... and measure() asks it before looking at the fiducials
        PStMeasurer(fs=60000).measure(torch.zeros(2, 100), None)


def _fiducials(R, cap, fs=360):
    from ecg_denoise_amd import Fiducials
    z = lambda *s: torch.zeros(*s, dtype=torch.int32)
    return Fiducials(z(R, cap), z(R, cap), z(R, cap), z(R, cap), z(R, cap), z(R), fs)


def test_host_refusals_need_no_device():
    from ecg_denoise_amd import Beats, PStMeasurer, RalError
    ms = PStMeasurer()
    x = torch.zeros(2, 2, 1000)
    with pytest.raises(RalError, match="PStMeasurer.measure runs on the GPU: pass a device tensor"):
        ms.measure(x, _fiducials(2, 4))
    with pytest.raises(RalError, match="PStMeasurer.measure runs on the GPU: pass a device tensor"):
        ms.measure(np.zeros((2, 2, 1000), np.float32), _fiducials(2, 4))
    for bad in (torch.zeros(1000), torch.zeros(2, 2, 2, 1000), torch.zeros(2, 2, 0)):
        with pytest.raises(RalError, match=r"PStMeasurer.measure: expected \(leads, T\) or \(R, leads, T\)"):
            ms.measure(bad, _fiducials(2, 4))
    for R in (1, 3):
        with pytest.raises(RalError, match=rf"PStMeasurer.measure: {R} beat lists on cpu for 2 records on cpu"):
            ms.measure(x, _fiducials(R, 4))
    f = _fiducials(2, 4)
    f.on = f.on[:, :3]                                            # a cap that is not that of the positions
    with pytest.raises(RalError, match=r"PStMeasurer.measure: fiducials whose `on` is \(2, 3\)"):
        ms.measure(x, f)
    with pytest.raises(RalError, match="PStMeasurer.measure: fiducials at fs=500 for a measurement at fs=360"):
        ms.measure(x, _fiducials(2, 4, fs=500))
    for other in ([[5], [7]], Beats(torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32))):
        with pytest.raises(RalError, match="PStMeasurer.measure: expected the Fiducials of BeatDelineator.delineate"):
            ms.measure(x, other)
    for p0 in (float("nan"), float("inf"), -0.01):
        with pytest.raises(RalError, match="PStMeasurer.measure: need a finite p0 >= 0"):
            PStMeasurer(p0=p0)
    assert PStMeasurer(p0=0).p0 == 0.0


@functools.lru_cache(maxsize=None)
def _oracle():
    """-> (records, beats, labels, per record the oracle's (on, off, pon, ppeak, poff, st))"""
    from ecg_denoise_amd import synth
    x, beats, labels = synth.make_records_with_rhythm(4, 2, T, seed=SEED, p_v=0.15)
    return x, beats, labels, [P.delineate_and_measure(x[r], beats[r]) for r in range(4)]


def test_normal_beats_have_a_p_wave_in_front_of_the_qrs_and_ventricular_beats_have_none():
    x, beats, labels, res = _oracle()
    normal = found = ventricular = 0
    for pos, lab, (on, off, pon, ppeak, poff, st) in zip(beats, labels, res):
        for i, p in enumerate(pos):
            if lab[i] != 0:
                ventricular += 1
                assert (pon[i], ppeak[i], poff[i]) == (-1, -1, -1), (i, p)
            elif on[i] >= 0 and i >= 1:
                normal += 1
                found += ppeak[i] >= 0
            if ppeak[i] >= 0:
                assert 0 <= pon[i] < ppeak[i] < poff[i] < on[i], (i, p, pon[i], ppeak[i], poff[i], on[i])
                assert 100.0 <= (on[i] - pon[i]) * 1000.0 / FS <= 280.0, (i, p)          # PR
            else:
                assert (pon[i], ppeak[i], poff[i]) == (-1, -1, -1)
    assert normal >= 40 and ventricular >= 5
    assert found >= 0.9 * normal, (found, normal)


@pytest.mark.parametrize("k", [2.0, -1.0, 0.5])
def test_scaling_the_record_keeps_the_integers_and_scales_st_exactly(k):
    x, beats, labels, res = _oracle()
    seen = 0
    for r in range(4):
        on, off, pon, ppeak, poff, st = res[r]
        got = P.measure_record(x[r] * np.float32(k), beats[r], on, off)
        assert got[:3] == (pon, ppeak, poff)
        assert np.array_equal(np.isnan(got[3]), np.isnan(st))
        ok = ~np.isnan(st)
        assert np.array_equal(got[3][ok], st[ok] * np.float32(k))
        seen += int(ok[:, 0].sum())
    assert seen >= 40


@pytest.mark.parametrize("c", [0.2, -0.2])
def test_an_st_deviation_on_one_lead_moves_the_st_level_of_that_lead(c):
    """c exp(-0.5 ((t - p / fs - 0.11) / 0.035)^2) added to lead 0 at every beat, the records delineated again: on every normal
    beat whose ST can be read in both, st[0] moves by 0.8 to 1.0 of c and st[1] by at most 0.01.  The bump is centred 110 ms
    behind the R peak, which is J + 60 ms of a narrow QRS only: a ventricular beat's J point lies some 50 ms later, its ST
    sample on the bump's tail (0.16 to 0.33 of c in these records), so the claim is made of the normal beats."""
    x, beats, labels, res = _oracle()
    y = x.astype(np.float64)
    t = np.arange(T) / FS
    for r in range(4):
        for p in beats[r]:
            y[r, 0] += c * np.exp(-0.5 * ((t - p / FS - 0.11) / 0.035) ** 2)
    y = y.astype(np.float32)
    seen = 0
    for r in range(4):
        st0, st1 = res[r][5], P.delineate_and_measure(y[r], beats[r])[5]
        for i in range(len(beats[r])):
            if np.isnan(st0[i, 0]) or np.isnan(st1[i, 0]) or labels[r][i] != 0:
                continue
            d = (st1[i].astype(np.float64) - st0[i]) / c
            assert 0.8 <= d[0] <= 1.0 and abs(d[1] * c) <= 0.01, (r, i, d)
            seen += 1
    assert seen >= 45


def test_the_oracle_at_the_edges():
    x, beats, labels, res = _oracle()
    G = P.geometry(FS)
    nan2 = [True, True]
    flat = P.measure_beat(np.full((2, 300), 3.0, np.float32), 150, 140, 160)                    # constant: s == 0 everywhere,
    assert flat[:3] == (-1, -1, -1) and flat[3].tolist() == [0.0, 0.0]                          # no P, and an ST level of 0
    one = P.measure_beat(x[0][:, :1].copy(), 0, 0, 0)                                           # T = 1: ts = j > lim = 0
    assert one[:3] == (-1, -1, -1) and np.isnan(one[3]).tolist() == nan2
    # a beat with all its points, the first normal beat behind a normal beat
    r, i = next((r, i) for r in range(4) for i in range(1, len(beats[r])) if res[r][3][i] >= 0 and not np.isnan(res[r][5][i, 0]))
    p, on, off = beats[r][i], res[r][0][i], res[r][1][i]
    whole = P.measure_beat(x[r], p, on, off, beats[r][i - 1], beats[r][i + 1])
    assert whole[:3] == (res[r][2][i], res[r][3][i], res[r][4][i]) and whole[1] >= 0
    for bad_on in (-1, p + 1, -5):                                                              # on missing: nothing is measured
        miss = P.measure_beat(x[r], p, bad_on, off, beats[r][i - 1], beats[r][i + 1])
        assert miss[:3] == (-1, -1, -1) and np.isnan(miss[3]).tolist() == nan2
    for bad_off in (-1, p - 1, T):                                                              # off missing: the P wave stays,
        miss = P.measure_beat(x[r], p, on, bad_off, beats[r][i - 1], beats[r][i + 1])           # S is taken over [on, p]
        assert miss[:3] == whole[:3] and np.isnan(miss[3]).tolist() == nan2
    alone = P.measure_beat(x[r], p, on, off, beats[r][i - 1])                                   # a distant next beat changes nothing
    assert alone[:3] == whole[:3] and P.same_bits(alone[3], whole[3])
    # two beats half a QRS window apart: the second one's P search starts at 2/3 of their distance, behind its isoelectric
    # sample: plo > phi, no P wave - and the first one's ST sample lies behind the 2/3 cap: no ST level
    half = U.geometry(FS)["Wq"] // 2
    on2 = U.delineate_beat(x[r], p + half)[0]
    assert on2 >= 0 and p + (2 * half) // 3 > max(on2 - G["g"], 0)
    second = P.measure_beat(x[r], p + half, on2, U.delineate_beat(x[r], p + half)[1], prev=p)
    assert second[:3] == (-1, -1, -1)
    first = P.measure_beat(x[r], p, on, off, beats[r][i - 1], p + half)
    assert first[:3] == whole[:3] and np.isnan(first[3]).tolist() == nan2 and off + G["j"] > p + (2 * half) // 3
    # a first beat near sample 0: the search is cut to the record, [0, on - g], and an onset within g of the start leaves a
    # window of one sample, whose argmax lies on its edge
    cut = x[r][:, p - 60:].copy()
    near = P.measure_beat(cut, 60, on - (p - 60), off - (p - 60))
    assert near[:3] == (-1, -1, -1) or 0 <= near[0] < near[1] < near[2] < on - (p - 60)
    assert not np.isnan(near[3]).any()
    tight = P.measure_beat(x[r][:, on - 3:].copy(), p - on + 3, 3, off - on + 3)
    assert tight[:3] == (-1, -1, -1) and not np.isnan(tight[3]).any()
