"""Beat delineation without a device: the geometry, the host-side refusals, and what the numpy oracle (tests/delineate_util.py)
says about the synthetic rhythm records - the properties that make the definition a delineator, checked on the oracle alone."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

import delineate_util as U

T, FS = 3600, 360
SEED = 24          # (checked with the oracle alone: every claim below holds for these four records)


@pytest.mark.parametrize("fs,want", [
    (360, dict(h=2, m=3, Wq=43, g=7, m2=6, gt=22, Wt=198)),
    (500, dict(h=3, m=4, Wq=60, g=10, m2=8, gt=30, Wt=275)),
    (250, dict(h=1, m=2, Wq=30, g=5, m2=4, gt=15, Wt=138)),          # 137.5 rounds up
    (1000, dict(h=6, m=8, Wq=120, g=20, m2=17, gt=60, Wt=550)),
])
def test_geometry(fs, want):
    from ecg_denoise_amd import delineate_check, delineate_geometry
    assert delineate_geometry(fs) == want == U.geometry(fs)
    assert delineate_geometry(Fraction(fs)) == want
    assert delineate_check(fs, 12) == want
    assert delineate_geometry(90)["h"] == 1          # (round(0.5) = 1 and the floor of 1 agree; below that the floor holds)
    assert delineate_geometry(45)["h"] == 1


def test_check_refuses_an_oversized_rate_before_touching_the_library(monkeypatch):
    from ecg_denoise_amd import BeatDelineator, RalError, _lib, delineate_check

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_library)
    with pytest.raises(RalError, match="fs=20000 is not supported.*64 KB of LDS"):
        delineate_check(20000, 2)
    for leads in (0, 65536, True, 2.0):
        with pytest.raises(RalError, match="leads"):
            delineate_check(360, leads)
    assert delineate_check(8000, 2)["Wt"] == 4400
    with pytest.raises(RalError, match="not supported"):          # ... and delineate() asks it before anything else
        BeatDelineator(fs=20000).delineate(torch.zeros(2, 100), [[5]])
    with pytest.raises(RalError, match="q0"):
        BeatDelineator(q0=float("nan"))


@functools.lru_cache(maxsize=None)
def _oracle():
    """-> (records, beats, labels, the oracle's four lists per record)"""
    from ecg_denoise_amd import synth
    x, beats, labels = synth.make_records_with_rhythm(4, 2, T, seed=SEED, p_v=0.15)
    return x, beats, labels, [U.delineate_record(x[r], beats[r]) for r in range(4)]


def test_every_beat_inside_the_record_has_its_qrs_bounds_around_it():
    x, beats, labels, fid = _oracle()
    G = U.geometry(FS)
    ext = G["Wq"] + G["g"] + G["m"] + G["h"]
    seen = 0
    for pos, (on, off, _, _) in zip(beats, fid):
        for i, p in enumerate(pos):
            if p - ext >= 0 and p + ext <= T - 1:
                assert 0 <= on[i] < p < off[i], (i, p, on[i], off[i])
                assert p - G["Wq"] <= on[i] and off[i] <= p + G["Wq"]
                seen += 1
    assert seen >= 40 and {l for row in labels for l in row} == {0, 1}


def test_every_normal_beat_with_a_whole_t_window_has_a_t_wave_behind_its_qrs():
    """a normal beat followed by a normal beat, whose search window [off + gt, p + Wt] is cut neither by the 2/3 cap of the next
    beat nor by the record's end; V beats and the sinus beats before them carry no such claim"""
    x, beats, labels, fid = _oracle()
    G = U.geometry(FS)
    seen = 0
    for pos, lab, (on, off, tpeak, tend) in zip(beats, labels, fid):
        for i, p in enumerate(pos):
            last = i + 1 >= len(pos)
            if lab[i] != 0 or (not last and lab[i + 1] != 0) or p - G["Wq"] - G["g"] - G["m"] - G["h"] < 0:
                continue
            if p + G["Wt"] + G["m2"] > T - 1 or (not last and p + (2 * (pos[i + 1] - p)) // 3 < p + G["Wt"]):
                continue
            assert 0 <= off[i] < tpeak[i] < tend[i] <= p + G["Wt"], (i, p, off[i], tpeak[i], tend[i])
            seen += 1
    assert seen >= 6


def test_ventricular_beats_are_wider_than_normal_ones():
    x, beats, labels, fid = _oracle()
    records = 0
    for pos, lab, (on, off, _, _) in zip(beats, labels, fid):
        q = {k: [1000.0 * (b - a) / FS for a, b, l in zip(on, off, lab) if l == k and a >= 0 and b >= 0] for k in (0, 1)}
        if lab.count(1) >= 2 and lab.count(0) >= 2:
            assert len(q[0]) >= 2 and len(q[1]) >= 2
            assert np.median(q[1]) > np.median(q[0]) + 40.0, (np.median(q[0]), np.median(q[1]))
            assert 70.0 < np.median(q[0]) < 110.0 and 130.0 < np.median(q[1]) < 190.0
            records += 1
    assert records >= 2


def test_the_oracle_at_the_edges():
    x = _oracle()[0][0]
    assert U.delineate_beat(np.full((2, 50), 3.0, np.float32), 20) == (-1, -1, -1, -1)          # constant: A == 0
    assert U.delineate_beat(x[:, :1].copy(), 0) == (-1, -1, -1, -1)                             # T = 1
    short = U.delineate_beat(x[:, 120:150].copy(), 15)                                          # T < Wq around an R peak:
    assert short[2:] == (-1, -1) and all(-1 <= v < 30 for v in short)                           # off + gt lies past the record
    p = _oracle()[1][0][3]
    alone, capped = U.delineate_beat(x, p), U.delineate_beat(x, p, p + 21)                      # 2/3 cap: lim = p + 14 < off + gt
    assert alone[:2] == capped[:2] and capped[2:] == (-1, -1) and alone[2] > 0


def test_host_refusals_need_no_device():
    from ecg_denoise_amd import BeatDelineator, RalError
    dl = BeatDelineator()
    x = torch.zeros(2, 2, 1000)
    with pytest.raises(RalError, match="device tensor"):
        dl.delineate(x, [[5], [7]])
    with pytest.raises(RalError, match="device tensor"):
        dl.delineate(np.zeros((2, 2, 1000), np.float32), [[5], [7]])
    for bad in (torch.zeros(1000), torch.zeros(2, 2, 2, 1000), torch.zeros(2, 2, 0)):
        with pytest.raises(RalError, match=r"BeatDelineator.delineate: expected \(leads, T\) or \(R, leads, T\)"):
            dl.delineate(bad, [[5], [7]])
    for beats in ([[9, 3], [1]], [[5, 5], [1]], [[-1], [1]], [[1], [1000]]):
        with pytest.raises(RalError, match=r"BeatDelineator.delineate: the beats of a record must be strictly ascending positions in \[0, 1000\)"):
            dl.delineate(x, beats)
    for beats in ([[5]], [[5], [6], [7]]):
        with pytest.raises(RalError, match=rf"BeatDelineator.delineate: {len(beats)} beat lists for 2 records"):
            dl.delineate(x, beats)
    # the classifier and the detector check in the same order: shape, geometry, beat lists, and only then the device
    from ecg_denoise_amd import BeatClassifier, BeatDetector
    cl, det = BeatClassifier(), BeatDetector()
    with pytest.raises(RalError, match="device tensor"):
        cl.classify(x, [[5], [7]])
    with pytest.raises(RalError, match="device tensor"):
        cl.classify(np.zeros((2, 2, 1000), np.float32), [[5], [7]])
    for bad in (torch.zeros(1000), torch.zeros(2, 2, 2, 1000), torch.zeros(2, 2, 0)):
        with pytest.raises(RalError, match=r"BeatClassifier.classify: expected \(leads, T\) or \(R, leads, T\)"):
            cl.classify(bad, [[5], [7]])
    for beats in ([[9, 3], [1]], [[5, 5], [1]], [[-1], [1]], [[1], [1000]]):
        with pytest.raises(RalError, match=r"BeatClassifier.classify: the beats of a record must be strictly ascending positions in \[0, 1000\)"):
            cl.classify(x, beats)
    for beats in ([[5]], [[5], [6], [7]]):
        with pytest.raises(RalError, match=rf"BeatClassifier.classify: {len(beats)} beat lists for 2 records"):
            cl.classify(x, beats)
    with pytest.raises(RalError, match="device tensor"):
        det.detect(x)
    with pytest.raises(RalError, match="device tensor"):
        det.detect(np.zeros((2, 2, 1000), np.float32))
    for bad in (torch.zeros(1000), torch.zeros(2, 2, 2, 1000), torch.zeros(2, 2, 0)):
        with pytest.raises(RalError, match=r"BeatDetector.detect: expected \(leads, T\) or \(R, leads, T\)"):
            det.detect(bad)
    with pytest.raises(RalError, match="beat detection at fs=360 with 64 leads is not supported"):
        det.detect(torch.zeros(64, 1000))                    # a geometry that is refused, on a host tensor


def test_the_classifier_keeps_its_own_name_in_the_shared_messages():
    from ecg_denoise_amd import RalError
    from ecg_denoise_amd.intake import beat_lists
    what = "BeatClassifier.classify"
    with pytest.raises(RalError, match=r"^BeatClassifier.classify: 1 beat lists for 2 records$"):
        beat_lists([[5]], torch.device("cpu"), what, T=1000, R=2)
    with pytest.raises(RalError, match=r"^BeatClassifier.classify: the beats of a record must be strictly ascending positions in \[0, 1000\)$"):
        beat_lists([[9, 3], [1]], torch.device("cpu"), what, T=1000, R=2)
