"""On-the-fly noise mixing without a GPU: the restated Philox against the Random123 known answers, the statistics of the draw,
the library's own draw (ral_mix_draw: the code the kernel runs, on the host) against the restatement, the argument checks of
ral_mix_batch (they run before any device call) and the host side of `ecg_denoise_amd.augment`."""
import ctypes as C
import math

import numpy as np
import pytest

from augment_util import draw_ref, make_case, mix_ref, philox4x32_10, ulp_distance
from ecg_denoise_amd import NoiseMixSampler, RalError, _lib, kind_thresholds

PTR = C.c_void_p(0x1000)        # never dereferenced: every ral_mix_batch call below is refused before anything is launched


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_restated_philox_reproduces_the_random123_known_answers(counter, key, want):
    assert philox4x32_10(counter, key) == want


def test_draw_statistics():
    B, w = 4096, (0.5, 0.3, 0.2)
    N, Lsrc, L, Tn, lo, hi = 1000, 900, 512, 650000, -4.0, 4.0
    draws, snr = draw_ref(2023, 0, B, N, Lsrc, L, Tn, kind_thresholds(w), lo, hi)
    counts = np.bincount(draws[:, 2], minlength=3)
    assert counts.tolist() == [2098, 1208, 790]
    for k in range(3):
        assert abs(counts[k] - B * w[k]) <= 5 * math.sqrt(B * w[k] * (1 - w[k])), counts
    assert (snr >= lo).all() and (snr < hi).all() and snr.min() < -3.9 and snr.max() > 3.9
    for col, span in ((0, N), (1, Lsrc - L + 1), (3, Tn - L + 1)):
        v = draws[:, col]
        assert v.min() >= 0 and v.max() < span and (v < span // 2).any() and (v >= span // 2).any(), (col, v.min(), v.max())


def _draw(N, Lsrc, L, Tn, cum, lo, hi, seed, g):
    c = (C.c_uint32 * len(cum))(*cum)
    d, snr = (C.c_int32 * 4)(), C.c_double()
    rc = _lib.lib().ral_mix_draw(N, Lsrc, L, len(cum), Tn, c, lo, hi, seed, g, d, C.byref(snr))
    assert rc == 0, _lib.lib().ral_last_error().decode()
    return [d[0], d[1], d[2], d[3]], snr.value


@pytest.mark.parametrize("N,Lsrc,L,Tn,weights,seed,first", [
    (1, 16, 16, 16, (1.0,), 2023, 0),                                  # every range is a single value
    (7, 200, 48, 1000, (0.5, 0.3, 0.2), 2023, 100),
    (5, 64, 64, 300, (1, 0, 2), 0xfedcba9876543210, 2 ** 32 - 3),      # a 64-bit seed; the high counter word changes
    (2 ** 31 - 1, 5000, 512, 650000, (1,) * 8, 7, 2 ** 64 - 2),        # the largest bank; the ordinal wraps
])
def test_library_draw_is_the_restated_draw(N, Lsrc, L, Tn, weights, seed, first):
    cum = kind_thresholds(weights)
    want, wsnr = draw_ref(seed, first, 6, N, Lsrc, L, Tn, cum, -4.0, 30.0)
    for i in range(6):
        got, snr = _draw(N, Lsrc, L, Tn, cum, -4.0, 30.0, seed, (first + i) % 2 ** 64)
        assert got == want[i].tolist() and abs(snr - wsnr[i]) <= 1e-12, (i, got, want[i], snr, wsnr[i])


def _mix(N=10, leads=2, Lsrc=600, L=512, K=3, Tn=5000, cum=(2 ** 30, 2 ** 31, 2 ** 32 - 1), lo=-4.0, hi=4.0, B=4, bank=PTR,
         rows=None, draws=PTR, cum_ptr=True):
    c = (C.c_uint32 * 8)(*cum)
    rc = _lib.lib().ral_mix_batch(bank, PTR, rows, N, leads, Lsrc, L, K, Tn, c if cum_ptr else None, lo, hi, 2023, 0, B, PTR, PTR,
                                  draws, PTR, None)
    return rc, _lib.lib().ral_last_error().decode()


@pytest.mark.parametrize("kw,rule", [
    (dict(bank=None), "null pointer"), (dict(draws=None), "null pointer"), (dict(cum_ptr=False), "null pointer"),
    (dict(N=0), "N >= 1"),
    (dict(leads=0), "1 <= leads <= 16"), (dict(leads=17, L=64), "1 <= leads <= 16"),
    (dict(L=0), "1 <= L <= Lsrc"), (dict(L=601), "1 <= L <= Lsrc"),
    (dict(K=0), "1 <= K <= 8"), (dict(K=9), "1 <= K <= 8"),
    (dict(Tn=511), "Tn >= L"),
    (dict(B=0), "B >= 1"),
    (dict(lo=float("nan")), "finite snr_lo <= snr_hi"), (dict(hi=float("inf")), "finite snr_lo <= snr_hi"),
    (dict(lo=4.0, hi=-4.0), "finite snr_lo <= snr_hi"),
    (dict(cum=(2 ** 31, 2 ** 30, 2 ** 32 - 1)), "non-decreasing thresholds"),
    (dict(N=2 ** 31), "N < 2^31"), (dict(Tn=2 ** 32 + 511), "Tn - L + 1 < 2^32"), (dict(B=2 ** 31), "B < 2^31"),
    (dict(leads=12, Lsrc=2048, L=1376), "leads * L <= 16384"), (dict(leads=1, Lsrc=16385, L=16385, Tn=20000), "leads * L <= 16384"),
])
def test_mix_batch_refuses_each_broken_rule_by_name_before_any_device_call(kw, rule):
    rc, msg = _mix(**kw)
    assert rc != 0 and msg.startswith("mix_batch: need ") and rule in msg, msg
    assert "N=" in msg and "Tn=" in msg, msg                            # the values follow the rule


def test_thresholds_from_weights():
    assert kind_thresholds([3.0]) == [0xFFFFFFFF]                                  # K = 1: nothing to draw
    assert kind_thresholds([1, 1]) == [2 ** 31, 0xFFFFFFFF]
    assert kind_thresholds([0.5, 0.3, 0.2]) == [2 ** 31, math.floor(2 ** 32 * 0.8), 0xFFFFFFFF]
    assert kind_thresholds([2, 0, 2]) == [2 ** 31, 2 ** 31, 0xFFFFFFFF]              # a zero weight: an empty interval
    assert kind_thresholds([0, 0, 5]) == [0, 0, 0xFFFFFFFF]
    assert kind_thresholds([1, 0]) == [0xFFFFFFFF, 0xFFFFFFFF]                       # 2^32 does not fit: clamped
    draws, _ = draw_ref(1, 0, 2000, 10, 64, 64, 100, kind_thresholds([2, 0, 2]), 0.0, 1.0)
    assert set(draws[:, 2].tolist()) == {0, 2}
    for bad in ([], [1] * 9, [-1, 2], [0, 0], [float("nan"), 1]):
        with pytest.raises(RalError):
            kind_thresholds(bad)


def _sampler(**kw):
    bank, noise = make_case(6, 2, 80, 3, 400, seed=3)
    args = dict(L=64, snr_db=(-4.0, 4.0), weights=(0.5, 0.3, 0.2), seed=2023)
    args.update(kw)
    return NoiseMixSampler(bank, {"bw": noise[0], "ma": noise[1], "em": noise[2]}, **args)


def test_sampler_shards_and_positions():
    one = _sampler()
    assert one.kinds == ("bw", "ma", "em") and (one.N, one.leads, one.Lsrc, one.L, one.K, one.Tn) == (6, 2, 80, 64, 3, 400)
    assert one.position == 0 and one.advance(10) == 0 and one.position == 10 and one.advance(4) == 10 and one.position == 14
    r0, r1 = _sampler(rank=0, world=2), _sampler(rank=1, world=2)
    assert (r0.advance(5), r1.advance(5)) == (0, 5) and r0.position == r1.position == 10       # [0, 5) and [5, 10) of one batch of 10
    assert (r0.advance(3), r1.advance(3)) == (10, 13) and r0.position == r1.position == 16
    # a replay loader sets its ordinals aside when it is made; a plain one takes none until it is iterated
    s = _sampler(rank=1, world=2)
    val = s.loader(4, 3, replay=True)
    assert (val.start, len(val), s.position) == (0, 3, 24)
    tr = s.loader(4, 5)
    assert (tr.start, len(tr), s.position) == (None, 5, 24)
    # the position wraps with the 64-bit ordinal
    s.position = 2 ** 64 - 4
    assert s.advance(4) == 0 and s.position == 4
    # the host draw of an ordinal: what the restatement says
    want, wsnr = draw_ref(2023, 5, 1, 6, 80, 64, 400, one.thresholds, -4.0, 4.0)
    d = one.draw(5)
    assert list(d[:4]) == want[0].tolist() and abs(d[4] - wsnr[0]) <= 1e-12
    with pytest.raises(RalError, match="rank"):
        _sampler(rank=2, world=2)
    with pytest.raises(RalError, match="B >= 1"):
        one.advance(0)


def test_sampler_state_dict_round_trip():
    a = _sampler(seed=99)
    a.advance(7); a.advance(5)
    state = a.state_dict()
    assert state["seed"] == 99 and state["position"] == 12
    import json
    assert json.loads(json.dumps(state)) == state            # small, plain host values
    b = _sampler(seed=1)
    b.load_state_dict(state)
    assert (b.seed, b.position) == (99, 12) and b.state_dict() == state and b.advance(3) == a.advance(3)
    with pytest.raises(RalError, match="configured differently"):
        _sampler(L=48).load_state_dict(state)
    with pytest.raises(RalError, match="configured differently"):
        _sampler(weights=(1, 1, 1)).load_state_dict(state)


def test_sampler_refuses_bad_inputs_and_has_no_cpu_fallback():
    bank, noise = make_case(4, 2, 64, 3, 300, seed=1)
    with pytest.raises(RalError, match=r"one shape.*ma: \(2, 299\)"):
        NoiseMixSampler(bank, {"bw": noise[0], "ma": noise[1][:, :299], "em": noise[2]})
    with pytest.raises(RalError, match="no CPU fallback"):
        NoiseMixSampler(bank, noise, device="cpu")
    with pytest.raises(RalError, match="leads"):
        NoiseMixSampler(bank[:, :1], noise)
    with pytest.raises(RalError, match="weights"):
        NoiseMixSampler(bank, noise, weights=(1, 1))
    with pytest.raises(RalError, match="Tn >= L"):                     # the library's rules hold at construction
        NoiseMixSampler(bank, noise[:, :, :40])
    with pytest.raises(RalError, match="finite snr_lo <= snr_hi"):
        NoiseMixSampler(bank, noise, snr_db=(4.0, -4.0))
    s = NoiseMixSampler(bank, noise, weights={"noise0": 1, "noise1": 0, "noise2": 1})
    assert s.kinds == ("noise0", "noise1", "noise2") and s.L == 64 and s.thresholds == [2 ** 31, 2 ** 31, 0xFFFFFFFF]


def test_restated_mix_hits_the_asked_snr_and_handles_the_degenerate_inputs():
    bank, noise = make_case(3, 2, 100, 2, 500, seed=5)
    bank[1, 0] = 7.5                                                   # a constant lead
    noise[1, :, 100:164] = 0.0                                         # an all-zero noise segment
    draws = np.array([[0, 3, 0, 17], [1, 0, 0, 5], [2, 36, 1, 100]])
    snr = np.array([-4.0, 0.0, 30.0])
    noisy, clean = mix_ref(bank, noise, draws, snr, 64)
    assert np.isfinite(noisy).all() and np.isfinite(clean).all()
    assert (clean[1, 0] == 0).all() and np.array_equal(noisy[2], clean[2])
    c, e = clean.astype(np.float64), noisy.astype(np.float64) - clean.astype(np.float64)
    got = 10 * np.log10((c[:2] ** 2).sum((1, 2)) / (e[:2] ** 2).sum((1, 2)))
    assert np.abs(got - snr[:2]).max() < 1e-5
    assert abs(clean[0].astype(np.float64).std(axis=1) - 1).max() < 1e-6 and ulp_distance(clean[0], clean[0] + 0) == 0
