"""The median beat without a device: the geometry, the host-side and the library's refusals, what the numpy oracle
(tests/template_util.py) does at the edges of the definition, and - with the delineator's oracle (tests/delineate_util.py) - the
properties that make the median beat worth measuring on the synthetic rhythm records: it delineates where the single beats do,
and muscle noise moves it far less than it moves a single beat."""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

import delineate_util as D
import template_util as U


# ------------------------------------------------------------------------------------------------ 1. geometry and check
@pytest.mark.parametrize("fs,want", [
    (360, dict(Wpre=126, Wpost=234, Wn=361, W=3600, H=3600)),
    (500, dict(Wpre=175, Wpost=325, Wn=501, W=5000, H=5000)),
    (250, dict(Wpre=88, Wpost=163, Wn=252, W=2500, H=2500)),                       # 87.5 and 162.5 round up
    (Fraction(1000, 3), dict(Wpre=117, Wpost=217, Wn=335, W=3333, H=3333)),
])
def test_geometry(fs, want):
    from ecg_denoise_amd import template_check, template_geometry
    g = template_geometry(fs)
    assert g == dict(want, fs=Fraction(fs), KMAX=256) == U.geometry(fs)
    assert template_check(g, 12) is g
    g2 = template_geometry(fs, win_s=4, hop_s=0.5)
    assert g2["W"] == U._round(4 * Fraction(fs)) and g2["H"] == U._round(Fraction(fs) / 2) and g2 == U.geometry(fs, 4, Fraction(1, 2))


def test_check_refuses_before_touching_the_library(monkeypatch):
    from ecg_denoise_amd import MedianBeat, RalError, _lib, template_check, template_geometry

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_library)
    for leads in (0, 65536, True, 2.0):
        with pytest.raises(RalError, match="leads"):
            template_check(template_geometry(360), leads)
    for kw, rule in ((dict(fs=1), "1 <= Wpre <= 2\\^19 \\(Wpre=0"), (dict(fs=2 * 10 ** 6), "1 <= Wpre <= 2\\^19 \\(Wpre=700000"), (dict(win_s=0), "1 <= W < 2\\^31"),
                     (dict(win_s=10 ** 7), "1 <= W < 2\\^31"), (dict(hop_s=0.001), "1 <= H < 2\\^31")):
        with pytest.raises(RalError, match="median beat: this geometry is not supported: need " + rule):
            template_check(template_geometry(**kw), 2)
    with pytest.raises(RalError, match="1 <= KMAX <= 256"):
        template_check(dict(template_geometry(360), KMAX=257), 2)
    # average() asks in the order shape, geometry, beat lists, labels, device
    mb = MedianBeat(360)
    with pytest.raises(RalError, match=r"MedianBeat.average: expected \(leads, T\)"):
        mb.average(torch.zeros(4), [[1]])
    with pytest.raises(RalError, match="not supported: need 1 <= H"):
        MedianBeat(360, hop_s=0).average(torch.zeros(2, 100), [[5]])
    with pytest.raises(RalError, match="MedianBeat.average: the beats of a record must be strictly ascending"):
        mb.average(torch.zeros(2, 100), [[5, 5]])
    with pytest.raises(RalError, match="MedianBeat.average: 2 beat lists for 1 records"):
        mb.average(torch.zeros(2, 100), [[5], [6]])
    with pytest.raises(RalError, match="MedianBeat.average: one label per beat"):
        mb.average(torch.zeros(2, 100), [[5, 9]], [[0]])
    with pytest.raises(RalError, match="MedianBeat.average runs on the GPU"):
        mb.average(torch.zeros(2, 100), [[5, 9]], [[0, 1]])


# ------------------------------------------------------------------------------------------------ 2. the library's refusals
_PTRS = ("x", "geom", "peaks", "label", "count", "tpl", "used", "total", "rr")
_REFUSALS = (
    [({p: None}, f"{p} is NULL") for p in _PTRS if p != "label"]
    + [({"R": 0}, "R must be in [1, 65535]"), ({"R": 65536}, "R must be in [1, 65535]"),
       ({"leads": 0}, "leads must be in [1, 65535]"), ({"leads": 65536}, "leads must be in [1, 65535]"),
       ({"T": 0}, "T must be in [1, 2^31)"), ({"T": 2 ** 31}, "T must be in [1, 2^31)"),
       ({"cap": 0}, "cap must be in [1, 2^31)"), ({"cap": 2 ** 31}, "cap must be in [1, 2^31)"),
       ({"wpre": 0}, "geom.wpre must be in [1, 2^19]"), ({"wpre": 2 ** 19 + 1}, "geom.wpre must be in [1, 2^19]"),
       ({"wpost": 0}, "geom.wpost must be in [1, 2^19]"), ({"wpost": -3}, "geom.wpost must be in [1, 2^19]"),
       ({"w": 0}, "geom.w must be >= 1"), ({"h": 0}, "geom.h must be >= 1"),
       ({"kmax": 0}, "geom.kmax must be in [1, 256]"), ({"kmax": 257}, "geom.kmax must be in [1, 256]"),
       ({"nw": 0}, "nw must be max(1, (T - w) / h + 1)"), ({"nw": 2}, "nw must be max(1, (T - w) / h + 1)"),
       ({"nw": 4}, "nw must be max(1, (T - w) / h + 1)"), ({"nw": 1, "T": 700}, "nw must be max(1, (T - w) / h + 1)"),
       ({"nw": 2, "T": 50}, "nw must be max(1, (T - w) / h + 1)")])


@pytest.mark.parametrize("kw,msg", _REFUSALS, ids=["-".join(f"{k}={v}" for k, v in kw.items()) for kw, _ in _REFUSALS])
def test_the_entry_point_refuses_bad_arguments_before_any_launch(kw, msg):
    """ral_template_records refuses a null operand (label_or_null alone is optional), R, leads, T, cap out of range, a geometry
    out of range and an nw that is not the window rule's - each with a message that names the argument, and before any HIP
    call: this runs without a device (the operand pointers are host memory that a launch would fault on)"""
    from ecg_denoise_amd import _lib
    host = np.zeros(16, np.float32)
    a = dict(R=2, leads=2, T=1000, cap=4, nw=3, wpre=10, wpost=20, w=400, h=300, kmax=256)      # (1000 - 400) // 300 + 1 = 3
    ptr = {p: host.ctypes.data_as(C.c_void_p) for p in _PTRS}
    ptr["label"] = C.c_void_p(0)                                     # the optional operand is absent in every case
    for k, v in kw.items():
        if k in ptr:
            ptr[k] = C.c_void_p(0)
        else:
            a[k] = v
    geom = _lib.TemplateGeom(a["wpre"], a["wpost"], a["w"], a["h"], a["kmax"])
    L = _lib.lib()
    L.ral_param_floats(C.byref(_lib.make_config("full", 2, 512, 0, 1)))     # leaves another message behind
    rc = L.ral_template_records(ptr["x"], a["R"], a["leads"], a["T"], C.byref(geom) if ptr["geom"] else None, ptr["peaks"],
                                ptr["label"], ptr["count"], a["cap"], a["nw"], ptr["tpl"], ptr["used"], ptr["total"], ptr["rr"],
                                C.c_void_p(0))
    err = L.ral_last_error().decode()
    assert rc != 0 and err.startswith(f"ral_template_records: {msg}"), (rc, err)


# ------------------------------------------------------------------------------------------------ 3. the oracle's properties
def _noise_record(leads, T, seed=0):
    return np.random.default_rng(seed).standard_normal((leads, T)).astype(np.float32)


def test_a_record_of_identical_beats_gives_that_beat_bit_for_bit():
    g = U.geometry(360)
    beat = _noise_record(2, g["Wn"], 1)
    for n in (1, 2, 5, 8):
        T = n * g["Wn"] + 7
        x = np.zeros((2, T), dtype=np.float32)
        pos = [3 + g["Wpre"] + j * g["Wn"] for j in range(n)]
        for p in pos:
            x[:, p - g["Wpre"]:p + g["Wpost"] + 1] = beat
        out = U.median_beats(x, pos, None, g)
        assert out["used"].tolist() == [n] == out["total"].tolist() and out["rr"].tolist() == [g["Wn"] if n > 1 else -1]
        assert out["template"][0].tobytes() == beat.tobytes()


def test_labels_equal_the_lists_with_the_other_beats_removed_rr_apart():
    T = 3600
    g = dict(U.geometry(360), W=T, H=T)
    x = _noise_record(2, T, 2)
    pos = list(range(150, 3300, 97))
    lab = [(0, 0, 1, 0, 2, 0, -1)[i % 7] for i in range(len(pos))]
    a = U.median_beats(x, pos, lab, g)
    b = U.median_beats(x, [p for p, l in zip(pos, lab) if l == 0], None, g)
    for k in ("template", "used", "total"):
        assert np.array_equal(a[k], b[k]), k
    assert len(a["used"]) == 1 and 10 < a["used"][0] < len(pos)
    assert a["rr"].tolist() == [97] and b["rr"].tolist() == [194]      # (the previous beat of the LIST, whatever its label)
    none = U.median_beats(x, pos, [1] * len(pos), g)
    assert not none["template"].any() and none["used"].tolist() == [0] and none["rr"].tolist() == [-1]


def test_membership_boundaries_and_the_cap():
    g = U.geometry(360)
    T = 1000
    x = _noise_record(1, T, 3)
    pre, post = g["Wpre"], g["Wpost"]
    pos = [0, pre - 1, pre, T - 1 - post, T - post, T - 1]
    out = U.median_beats(x, pos, None, g)
    assert U.members(pos, None, T, 0, T, g) == [2, 3] and out["total"].tolist() == [2]
    want = (x[:, :g["Wn"]] + x[:, T - g["Wn"]:]) * np.float32(0.5)
    assert np.array_equal(out["template"][0], want) and out["rr"].tolist() == [1]           # sorted [1, T - 1 - post - pre]: the lower
    assert U.median_beats(x[:, :g["Wn"] - 1], [pre], None, g)["used"].tolist() == [0]       # T < Wn: no beat fits
    # the cap: 300 members, the first 256 are measured
    T = 1400
    x = _noise_record(1, T, 4)
    pos = list(range(pre, pre + 300))
    out = U.median_beats(x, pos, None, g)
    first = U.median_beats(x, pos[:256], None, g)
    assert out["total"].tolist() == [300] and out["used"].tolist() == [256] == first["total"].tolist()
    assert np.array_equal(out["template"], first["template"]) and out["rr"].tolist() == [1]
    assert not np.array_equal(out["template"], U.median_beats(x, pos[:255], None, g)["template"])
    # a window's members are its own: W = 400, H = 300 over T = 1000
    g2 = dict(g, W=400, H=300)
    assert U.windows(1000, g2) == [(0, 400), (300, 700), (600, 1000)] and U.windows(50, g2) == [(0, 50)]


# ------------------------------------------------------------------------------------------------ 4. with the delineator's oracle
# (the records of the delineator's tests: p_v = 0.15 for all three)
_SETS = {"360a": (3, 2, 3600, 24, 360), "360b": (3, 2, 7200, 5, 360), "500": (3, 12, 4000, 12, 500)}


@functools.lru_cache(maxsize=None)
def _set(name):
    """-> (records, beats, labels, fs, geometry with one whole-record window, the oracle's median beats)"""
    from ecg_denoise_amd import synth
    R, leads, T, seed, fs = _SETS[name]
    x, beats, labels = synth.make_records_with_rhythm(R, leads, T, seed=seed, p_v=0.15)
    g = dict(U.geometry(fs), W=T, H=T)
    return x, beats, labels, fs, g, U.median_beats_records(x, beats, labels, g)


@pytest.mark.parametrize("name", sorted(_SETS))
def test_the_median_beat_delineates_where_its_beats_do(name):
    """every template has all four points in order, and each within 4 samples of the median of the per-beat points of the N
    beats it was taken over (observed: at most 3)"""
    x, beats, labels, fs, g, med = _set(name)
    worst = 0
    for r in range(len(beats)):
        T = x.shape[2]
        use = U.members(beats[r], labels[r], T, 0, T, g)
        assert len(use) == med["used"][r, 0] >= 3
        on, off, tpeak, tend = D.delineate_beat(med["template"][r, 0], g["Wpre"], None, fs)
        assert 0 <= on < g["Wpre"] < off < tpeak < tend, (r, on, off, tpeak, tend)
        per = [D.delineate_beat(x[r], beats[r][i], beats[r][i + 1] if i + 1 < len(beats[r]) else None, fs) for i in use]
        for k, mine in enumerate((on, off, tpeak, tend)):
            rel = [f[k] - beats[r][i] + g["Wpre"] for f, i in zip(per, use) if f[k] >= 0]
            assert len(rel) >= 3
            worst = max(worst, abs(mine - float(np.median(rel))))
    print(f"{name}: the largest distance of a template's point from the median of the per-beat points is {worst} samples")
    assert worst <= 4


@pytest.mark.parametrize("name", sorted(_SETS))
def test_muscle_noise_at_0_db_moves_the_median_beat_less_than_half_as_far_as_a_single_beat(name):
    """`ma` noise at 0 dB (scale sqrt(P_sig / P_noise), the powers over the whole record and all leads): the RMSE of the noisy
    template against the clean template is at most 0.5 of the mean RMSE of the noisy single beats against it (observed: 0.19
    to 0.28)"""
    from ecg_denoise_amd import synth
    x, beats, labels, fs, g, med = _set(name)
    R, leads, T, seed = _SETS[name][:4]
    z = synth.make_noise_record("ma", leads, T, seed + 100).astype(np.float64)
    for r in range(R):
        xr = x[r].astype(np.float64)
        noisy = (xr + np.sqrt((xr ** 2).mean() / (z ** 2).mean()) * z).astype(np.float32)
        tn = U.median_beats(noisy, beats[r], labels[r], g)["template"][0].astype(np.float64)
        tc = med["template"][r, 0].astype(np.float64)
        single = [np.sqrt(((noisy[:, beats[r][i] - g["Wpre"]:beats[r][i] + g["Wpost"] + 1] - tc) ** 2).mean())
                  for i in U.members(beats[r], labels[r], T, 0, T, g)]
        ratio = np.sqrt(((tn - tc) ** 2).mean()) / np.mean(single)
        print(f"{name} record {r}: template RMSE / mean single-beat RMSE = {ratio:.3f} over {len(single)} beats")
        assert ratio <= 0.5
