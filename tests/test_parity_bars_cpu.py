"""The per-tensor parity bars (tests/parity_bars.py on RA-LENet's step, parity_util.parity_yardstick) on the CPU: the yardstick has
run_parity's keys, its values are usable, no existing case gets a weaker bar, every case keeps its distance from the stem's
LeakyReLU kink, the spread cases put GELU arguments into every part of [-10, 10] - and the bars reject what they are for:
the fp32 oracle with a GELU that is wrong by a relative 2e-6 (3e-6 beyond |x| = 3 only), which the flat bars let through."""
import math

import numpy as np
import pytest
import torch

import ralenet_oracle as O
import test_gpu_attention_t32 as A
import test_gpu_block_instances as I
import test_gpu_parity as P
from parity_bars import FWD_TOL, GRAD_TOL, K_PAIR, STEM_MARGIN, bars as parity_bars, check, errors, flat_bars, is_zero
from parity_util import parity_yardstick, spread_fc1_bias, stem_margin, step

PLAIN = ("full", 2, 256, 3)


def _values(cases):
    return [tuple(getattr(c, "values", c)) for c in cases]


# (variant, leads, L, B, params) of every case that is checked against a yardstick
EXISTING = ([c + (None,) for c in P.PLAIN_CASES + P.LENGTH_CASES] + [A.MODEL_CASE + (None,)]
            + [(v, 2, L, B, None) for v, L, B, _, _, spread in _values(I.CASES) if not spread])
SPREAD = list(dict.fromkeys([(v, leads, L, B, spread_fc1_bias) for v, leads, L, B, _ in _values(P.SPREAD_CASES)]
                            + [(v, 2, L, B, spread_fc1_bias) for v, L, B, _, _, spread in _values(I.CASES) if spread]))

_TRACE = (["a0", "x0", "blk0.out", "blk1.out", "p1", "blk2.out", "blk3.out", "p2", "blk4.out", "blk5.out", "p3", "blk6.out",
           "blk7.out", "p4", "blk8.out", "blk9.out", "xmid", "blk10.out", "blk11.out", "u3", "blk12.out", "blk13.out", "u2",
           "blk14.out", "blk15.out", "u1", "blk16.out", "blk17.out", "u0"])


def fp32_errors(variant, leads, L, B, params=None, eval_forward=False, gelu=None):
    """run_parity with the fp32 oracle in the place of the HIP path -> (errors against the fp64 oracle, the fp64 values);
    `gelu` replaces O.gelu in the fp32 evaluation only"""
    a, o = (step("ralenet", (variant, leads, L, B), dt, 2023, eval_forward=eval_forward, params=params, gelu=g)
            for dt, g in ((torch.float32, gelu), (torch.float64, None)))
    return errors(a.vals, o.vals), o.vals


def documented_keys(variant, leads, trace, eval_forward):
    """the keys of run_parity's result as its docstring and grad_values state them, from the parameter names alone"""
    keys = ["y", "loss", "snr", "rmse", "bn_mean", "bn_var"] + (["act:" + k for k in _TRACE] if trace else [])
    for k in O.ralenet_param_shapes(variant, leads):
        keys += ["grad:" + k + "[v]", "gradabs:" + k + "[k]"] if k.endswith("to_kv.bias") else ["grad:" + k]
    keys += ["grad:input"] + ["grad:%s@dx" % k for k in ("conv1.0.weight", "conv1.0.bias", "conv1.2.weight", "conv1.2.bias")]
    return keys + ["grad:input_frozen"] + (["y_eval"] if eval_forward else [])


@pytest.mark.parametrize("variant,leads,L,B", [("full", 2, 32, 2), ("nra", 1, 16, 2), ("mlp", 2, 32, 1)])
@pytest.mark.parametrize("trace,eval_forward", [(True, False), (False, False), (True, True), (False, True)])
def test_yardstick_has_the_keys_of_run_parity_and_usable_values(variant, leads, L, B, trace, eval_forward):
    yard = parity_yardstick(variant, leads, L, B, eval_forward=eval_forward, trace=trace)
    assert list(yard) == documented_keys(variant, leads, trace, eval_forward)
    ref = step("ralenet", (variant, leads, L, B), torch.float64, 2023).vals
    for k, v in yard.items():
        if k.startswith("gradabs:") or (k.startswith("grad:") and is_zero(ref[k])):
            assert v is None, k                                  # a true zero has no relative yardstick
        else:
            assert v is not None and math.isfinite(v) and v > 0, (k, v)
    assert yard["grad:input_frozen"] == yard["grad:input"] and yard["grad:conv1.0.bias@dx"] == yard["grad:conv1.0.bias"]
    bars = parity_bars(yard)
    assert list(bars) == list(yard) and all(math.isfinite(b) and b > 0 for b in bars.values())


@pytest.mark.parametrize("variant,leads,L,B", [PLAIN, ("mlp", 2, 256, 4), ("nra", 1, 16, 4), ("full", 2, 96, 2)])
def test_no_bar_of_an_existing_case_is_above_its_flat_bar(variant, leads, L, B):
    yard = parity_yardstick(variant, leads, L, B, eval_forward=True)
    bars = parity_bars(yard, K_PAIR, (FWD_TOL, GRAD_TOL))
    for k, b in bars.items():
        flat = GRAD_TOL if k.startswith("grad:") else FWD_TOL if not k.startswith("gradabs:") else 1e-5
        assert b <= flat, (k, b)
        assert b == flat if yard[k] is None else b >= K_PAIR * yard[k] or b == flat, (k, b, yard[k])
    # the bars are an order of magnitude or more below the flat ones where fp32 arithmetic is (the typical tensor)
    assert np.median([b for k, b in bars.items() if k.startswith("grad:") and yard[k] is not None]) < GRAD_TOL / 10
    assert np.median([b for k, b in bars.items() if not k.startswith(("grad:", "gradabs:"))]) <= FWD_TOL / 2


def test_bars_follow_the_rule():
    yard = {"y": 1e-7, "loss": 3e-7, "snr": 5e-7, "gradabs:b[k]": None, "grad:a": 1e-8, "grad:b": 2e-6, "grad:c": 3e-7,
            "grad:d": None, "grad:e": 1e-3}
    bars = parity_bars(yard)
    assert bars["y"] == 8 * 3e-7 and bars["loss"] == 8 * 3e-7 and bars["snr"] == 8 * 5e-7          # floored at the group median
    assert bars["gradabs:b[k]"] == 1e-5 and bars["grad:d"] == 1e-4                                  # no yardstick: the flat bar
    med = float(np.median([1e-8, 2e-6, 3e-7, 1e-3]))
    assert bars["grad:a"] == 8 * med and bars["grad:b"] == 8 * 2e-6 and bars["grad:e"] == 1e-4      # ... capped at the flat bar
    assert parity_bars(yard, capped=False)["grad:e"] == 8e-3 and parity_bars(yard, K=2.0)["grad:b"] == 4e-6


@pytest.mark.parametrize("variant,leads,L,B,params", list(dict.fromkeys(EXISTING + SPREAD)))
def test_every_case_keeps_its_distance_from_the_stem_kink(variant, leads, L, B, params):
    assert stem_margin(variant, leads, L, B, params=params) >= STEM_MARGIN


def test_every_yardstick_case_is_listed():
    assert len(EXISTING) == 8 + 9 + 1 + 6 and len(SPREAD) == 4          # (the twins share the spread full case's oracle)


@pytest.mark.parametrize("variant,leads,L,B,params", SPREAD)
def test_spread_cases_fill_the_gelu_range(variant, leads, L, B, params):
    """each 2-wide bin of [-10, 10] holds at least 2 % of the arguments O.gelu sees in the case, and everything stays finite"""
    args = []
    gelu = O.gelu

    def recording(x):
        args.append(x.detach().reshape(-1))
        return gelu(x)

    o = step("ralenet", (variant, leads, L, B), torch.float64, 2023, params=params, gelu=recording).vals
    a = torch.cat(args).numpy()
    share = np.histogram(a, bins=np.arange(-10.0, 10.5, 2.0))[0] / a.size
    print(variant, leads, L, B, "arguments %.1f .. %.1f, bins" % (a.min(), a.max()), np.round(100 * share, 1), "loss %.3f" % o["loss"])
    assert share.min() >= 0.02, share
    assert a.min() < -10 and a.max() > 10
    assert math.isfinite(o["loss"]) and all(np.isfinite(g).all() for k, g in o.items() if k.startswith("grad"))
    # ... where the seeded parameters alone stay below 3
    del args[:]
    step("ralenet", (variant, leads, L, B), torch.float64, 2023, gelu=recording)
    assert torch.cat(args).abs().max().item() < 3.0


def _gelu_off_by(eps, beyond):
    def gelu(x):
        return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0)))) * (1.0 + eps * (x.abs() > beyond))
    return gelu


def test_the_bars_reject_a_gelu_that_is_wrong_by_2e_6_and_the_flat_bars_do_not():
    yard = parity_yardstick(*PLAIN, eval_forward=True)
    exact, ref = fp32_errors(*PLAIN, eval_forward=True)
    check(exact, flat_bars(ref))
    check(exact, parity_bars(yard), yard)
    mutant, _ = fp32_errors(*PLAIN, eval_forward=True, gelu=_gelu_off_by(2e-6, -1.0))
    check(mutant, flat_bars(ref))                                      # invisible to the flat bars
    with pytest.raises(AssertionError, match=r"tensors above their bars") as e:
        check(mutant, parity_bars(yard), yard)
    assert int(str(e.value).split()[0]) > 100, str(e.value)[:200]      # (274 .. 286 of 330, by torch's thread count)
    # beyond |x| = 3 no argument of a plain case exists: nothing changes at all
    assert fp32_errors(*PLAIN, eval_forward=True, gelu=_gelu_off_by(1e-4, 3.0))[0] == exact


def test_the_bars_reject_a_gelu_that_is_wrong_by_3e_6_beyond_3_on_the_spread_case():
    yard = parity_yardstick(*PLAIN, params=spread_fc1_bias, eval_forward=True)
    bars = parity_bars(yard, capped=False)
    check(fp32_errors(*PLAIN, params=spread_fc1_bias, eval_forward=True)[0], bars, yard)
    mutant, _ = fp32_errors(*PLAIN, params=spread_fc1_bias, eval_forward=True, gelu=_gelu_off_by(3e-6, 3.0))
    with pytest.raises(AssertionError, match=r"tensors above their bars") as e:
        check(mutant, bars, yard)
    assert int(str(e.value).split()[0]) > 100, str(e.value)[:200]
    assert "yardstick" in str(e.value) and "bar" in str(e.value) and "grad:" in str(e.value)
