"""The per-tensor bars of the baseline networks and the 12-lead adapter (tests/baseline_parity_util.py: the rule of
tests/parity_bars.py on the steps of tests/parity_util.py) on the CPU: the
yardsticks have the keys the GPU tests compare, no bar is above the flat bar its case had, the kink precondition holds for every
case that takes per-tensor bars (and fails where CASES says it does), and the bars reject what they are for - an fp32 oracle
with a small defect that the flat bars let through:

  network   case               defect                                             above its bar   largest error (forward, gradient)
  U-Net     (2, 48, 5) @2024   BatchNorm eps 1.02e-5 for 1e-5                     26 of 65        5.8e-6, 4.0e-5
  ACDAE     (64, 3)            middle tap of the 13-tap convolution x (1 + 1e-5)  8 of 23         3.5e-6, 3.5e-6
  ACDAE     (64, 3)            upsample weights 0.249999 / 0.750001               1 of 23         1.4e-6, 1.5e-6
  DANet     (8, 32, 2) @10     BatchNorm eps 1.0015e-5                            62 of 202       3.6e-6, 7.0e-5
  DANet     (8, 32, 2) @10     every sigmoid x (1 + 3e-6)                         76 of 202       2.6e-6, 4.2e-5
  DANet     (8, 256, 2)        every sigmoid x (1 + 3e-6)                         5 of 202        2.5e-6, 4.2e-5
  adapter   (nra, 16, 4)       middle tap of the 13-tap convolutions x (1 + 1e-5) 9 of 15         7.9e-6, 9.1e-6
  adapter   (nra, 16, 4)       stem LeakyReLU slope 0.2 + 1e-5                    9 of 15         8.5e-6, 1.8e-5
(counts as measured with torch on one thread; the tests ask for at least one, and for none above the flat bars)"""
import math

import numpy as np
import pytest
import torch

import baseline_parity_util as U
import danet_oracle as D
import ralenet_oracle as O
from parity_bars import K_FP32, STEM_MARGIN, Kinks, check, errors, flat_bars, is_zero, yardstick
from parity_util import DANET_ZERO, step

NETS = ("unet", "acdae", "danet", "newrale")
BARRED = [(net,) + e for net in NETS for e in U.CASES[net] if e[2] is not None]
FLAT = [(net,) + e for net in NETS for e in U.CASES[net] if e[2] is None]
_id = lambda e: e[0] + "-" + U.case_id(e[0], e[1:])


def kinks(net, case, dtype, seed, mutant=None):
    return step(net, case, dtype, seed, mutant).kinks


def fp32_errors(net, case, seed, mutant=None):
    """errors with the fp32 oracle in the place of the HIP path; `mutant` changes the fp32 evaluation only"""
    return errors(step(net, case, torch.float32, seed, mutant).vals, step(net, case, torch.float64, seed).vals)


def documented_keys(net, case):
    """the keys of a GPU test's comparison, from the parameter names alone"""
    if net == "unet":
        stats = [k + s for k in O.UNET_BN for s in (".running_mean", ".running_var")]
        return ["y", "loss"] + stats + ["grad:" + k for k in O.unet_param_shapes(case[0])] + ["y_eval"]
    if net == "acdae":
        return ["y", "loss"] + ["grad:" + k for k in O.acdae_param_shapes()] + ["grad:input"]
    if net == "danet":
        sh = D.danet_state_shapes(case[2])
        return (["y_eval", "y", "loss", "grad:input"] + ["grad:" + k for k in sh if D.is_param(k) and ".dam.fcn2." not in k]
                + [k for k in sh if k.endswith(("running_mean", "running_var"))])
    return ["y", "loss", "snr", "rmse"] + ["grad:" + k for k in O.newrale_param_shapes()] + ["bn_mean", "bn_var", "y_eval"]


def test_the_cases_are_those_of_the_gpu_tests():
    """every shape the four tests had, each at its old input seed or - where that seed misses the precondition - at a seed that
    meets it AND at the old one under the flat bars; three new DANet shapes"""
    shapes = lambda net: list(dict.fromkeys(e[0] for e in U.CASES[net]))
    assert shapes("unet") == [(2, 512, 4), (1, 256, 3), (2, 1024, 2), (2, 48, 5), (2, 320, 3), (2, 64, 1025)]
    assert shapes("acdae") == [(512, 4), (256, 3), (1024, 2), (64, 3), (192, 2)]
    assert shapes("danet") == [(64, 512, 2), (37, 256, 2), (16, 1024, 2), (8, 512, 2), (4, 1024, 2), (8, 256, 2), (8, 32, 2), (4, 64, 2)]
    new = {(8, 512, 2): 20, (4, 1024, 2): 8}                      # new shapes have no old seed: theirs is what CASES gives them
    old_ids = {"unet": ["2-512-4", "1-256-3", "2-1024-2", "2-48-5", "2-320-3", "2-64-1025"],
               "acdae": ["512-4", "256-3", "1024-2", "64-3", "192-2"], "danet": ["64-512-2", "37-256-2", "16-1024-2", "8-32-2", "4-64-2"],
               "newrale": ["full-256-3", "nra-16-4", "full-32-2", "mlp-320-2", "nra-64-5", "full-1008-1", "nra-16-513"]}
    for net in NETS:                                              # ... and every old case keeps its id
        ids = [U.case_id(net, e) for e in U.CASES[net]]
        assert len(set(ids)) == len(ids) and set(old_ids[net]) <= set(ids), (net, ids)
    assert shapes("newrale") == [("full", 256, 3), ("nra", 16, 4), ("full", 32, 2), ("mlp", 320, 2), ("nra", 64, 5), ("full", 1008, 1),
                                 ("nra", 16, 513)]
    for net in NETS:
        for case in shapes(net):
            own = new.get(case, U.own_seed(net, case))
            mine = [(seed, seeds) for c, seed, seeds in U.CASES[net] if c == case]
            assert all(seeds is None or (seeds[0] == seed and len(set(seeds)) == 3) for seed, seeds in mine)
            at_own = [seeds for seed, seeds in mine if seed == own]
            moved = [seeds for seed, seeds in mine if seed != own]
            assert len(at_own) == 1 and len(moved) <= 1, (net, case)                      # the old input is still run
            assert all(s is not None for s in moved) and (not moved or at_own[0] is None), (net, case)
    assert len(BARRED) == 5 + 5 + 5 + 6 and len(FLAT) == 2 + 2 + 4 + 2


@pytest.mark.parametrize("net,case,seed,seeds", BARRED, ids=map(_id, BARRED))
def test_precondition_keys_and_bars_of_every_case_with_per_tensor_bars(net, case, seed, seeds):
    k = kinks(net, case, torch.float64, seed)
    assert k.margin >= STEM_MARGIN, (k.margin, k.where)
    assert all(kinks(net, case, torch.float32, s).same_sides(kinks(net, case, torch.float64, s)) for s in seeds)
    bars, yard = U.case_bars(net, case, seed, seeds)
    assert list(yard) == list(bars) == documented_keys(net, case)
    ref = step(net, case, torch.float64, seed).vals
    (fwd, grad), zero_abs = U.caps(net, case)
    assert (fwd, zero_abs) == (1e-5, 2e-5 if net == "unet" else 1e-5)
    assert grad == (2e-3 if net == "danet" and case[0] < 8 else 1e-4)
    zero = {k for k in yard if yard[k] is None}
    assert zero == {k for k, r in ref.items() if k.startswith("grad:") and is_zero(r)}
    if net == "danet":
        assert zero == {k for k in yard if k.endswith(DANET_ZERO)}
    elif net == "unet":       # the convolution biases in front of a batch-statistics BatchNorm; the old test's threshold was 1e-9
        assert zero == {"grad:%s.%d.conv.bias" % (s, i) for s in ("EncList", "DecList") for i in range(4)}
        assert all(np.linalg.norm(r) >= 1e-9 for k, r in ref.items() if k.startswith("grad:") and k not in zero)
    else:
        assert not zero
    for k, b in bars.items():
        if k in zero:
            assert b == zero_abs
            continue
        flat = grad if k.startswith("grad:") else fwd
        assert math.isfinite(yard[k]) and yard[k] > 0 and 0 < b <= flat, (k, yard[k], b)
        assert b >= K_FP32 * yard[k] or b == flat, (k, yard[k], b)
    # the typical bar is well below the flat one, and few bars are the flat one (DANet's gradients behind a BatchNorm over 4 or 8
    # descriptors are the least: the fp32 oracle's median gradient error is 6e-6 .. 9e-6 at B = 8, 7e-5 at B = 4)
    gb = [b for k, b in bars.items() if k.startswith("grad:") and k not in zero]
    fb = [b for k, b in bars.items() if not k.startswith("grad:")]
    assert np.median(gb) < grad / (2 if net == "danet" else 10) and np.median(fb) < fwd / 4
    assert sum(b == grad for b in gb) <= max(1, len(gb) / 10) and sum(b == fwd for b in fb) <= max(1, len(fb) / 10)   # (the adapter's SNR)
    # ... and the fp32 oracle itself is within them
    check(fp32_errors(net, case, seed), bars, yard)


@pytest.mark.parametrize("net,case,seed,seeds", FLAT, ids=map(_id, FLAT))
def test_cases_that_keep_their_flat_bars_miss_the_precondition(net, case, seed, seeds):
    margin = kinks(net, case, torch.float64, seed).margin
    assert margin < STEM_MARGIN, margin
    with pytest.raises(AssertionError):
        yardstick(lambda dtype, s: step(net, case, dtype, s), (seed, seed + 1, seed + 2))
    if net != "danet":
        bars, yard = U.case_bars(net, case, seed, None)
        assert yard is None and list(bars) == documented_keys(net, case)
        assert set(bars.values()) <= {1e-5, 1e-4, 2e-5}


def test_recording_sees_every_kink_and_leaves_the_oracles_as_they_were():
    before = (D.relu, D.clamp, D.sigmoid, D._bn, D.F, O.F)
    k = kinks("danet", (4, 64, 2), torch.float64, 4)
    kinds = [kind for kind, _ in k.sides]
    # per forward: 8 APReLUs (2 clamps and a ReLU each), 3 DAMs (2 ReLUs and 2 max-pools each); the eval and the train forward
    assert kinds.count("clamp") == 2 * 16 and kinds.count("relu") == 2 * (8 + 6) and kinds.count("adaptive_max_pool1d") == 2 * 6
    k = kinks("acdae", (64, 3), torch.float64, 2023)
    kinds = [kind for kind, _ in k.sides]
    assert kinds.count("max_pool1d") == 4 and kinds.count("leaky_relu") == 8
    assert k.count == 3 * (16 * 32 + 32 * 16 + 64 * 8 + 128 * 4) * 2 + 3 * (64 * 8 + 32 * 16 + 16 * 32 + 2 * 64)
    k = kinks("unet", (2, 48, 5), torch.float64, 2024)
    assert [kind for kind, _ in k.sides] == ["leaky_relu"] * 18                      # 4 + 2 + 3 per forward, train and eval
    k = kinks("newrale", ("nra", 16, 4), torch.float64, 2023)
    assert [kind for kind, _ in k.sides] == ["leaky_relu"] * 8                       # 3 of the adapter and the stem's, twice
    assert (D.relu, D.clamp, D.sigmoid, D._bn, D.F, O.F) == before
    assert D.relu is torch.relu and D.clamp is torch.clamp and D.sigmoid is torch.sigmoid


def test_a_kink_on_the_other_side_is_noticed():
    a, b = Kinks(), Kinks()
    x = torch.tensor([[[1.0, -2.0, 3e-9, 4.0]]], dtype=torch.float64)
    a.leaky_relu(x); a.max_pool1d(x, 2); a.adaptive_max_pool1d(x, 1)
    b.leaky_relu(x); b.max_pool1d(x, 2); b.adaptive_max_pool1d(x, 1)
    assert a.same_sides(b) and a.count == 4 + 2 + 1
    assert a.margin == pytest.approx(3e-9 / math.sqrt((1 + 4 + 16) / 4)) and a.where == "leaky_relu, call 0"
    c = Kinks()
    y = x.clone(); y[0, 0, 2] = -3e-9
    c.leaky_relu(y); c.max_pool1d(y, 2); c.adaptive_max_pool1d(y, 1)
    assert not a.same_sides(c)
    d = Kinks()
    z = torch.tensor([[[1.0, 1.0 + 1e-9, 0.5, 4.0]]], dtype=torch.float64)          # a pool pair 1e-9 apart
    d.max_pool1d(z, 2)
    assert d.margin < 1e-9 and d.where == "max_pool1d, call 0"
    e = Kinks()
    e.adaptive_max_pool1d(torch.tensor([[[4.0, 1.0, 4.0]]], dtype=torch.float64), 1)  # an exact tie
    assert e.margin == 0.0


MUTANT_CASES = [
    ("unet", (2, 48, 5), 2024, (2024, 2025, 2026), "unet_bn_eps"),
    ("acdae", (64, 3), 2023, (2023, 2024, 2025), "acdae_tap13"),
    ("acdae", (64, 3), 2023, (2023, 2024, 2025), "acdae_upsample"),
    ("danet", (8, 32, 2), 10, (10, 11, 12), "danet_bn_eps"),
    ("danet", (8, 32, 2), 10, (10, 11, 12), "danet_sigmoid"),
    ("danet", (8, 256, 2), 8, (8, 9, 10), "danet_sigmoid"),
    ("newrale", ("nra", 16, 4), 2023, (2023, 2024, 2025), "newrale_tap13"),
    ("newrale", ("nra", 16, 4), 2023, (2023, 2024, 2025), "newrale_stem_slope"),
]


@pytest.mark.parametrize("net,case,seed,seeds,mutant", MUTANT_CASES, ids=[m[0] + "-" + m[4] for m in MUTANT_CASES])
def test_the_bars_reject_a_small_defect_that_the_flat_bars_let_through(net, case, seed, seeds, mutant):
    assert (case, seed, seeds) in U.CASES[net]
    bars, yard = U.case_bars(net, case, seed, seeds)
    flat = flat_bars(step(net, case, torch.float64, seed).vals, *U.caps(net, case))
    err = fp32_errors(net, case, seed, mutant)
    # the defect moved no activation across a kink: what is measured is its arithmetic
    assert kinks(net, case, torch.float32, seed, mutant).same_sides(kinks(net, case, torch.float64, seed))
    check(err, flat)                                                   # invisible to the flat bars
    with pytest.raises(AssertionError, match=r"tensors above their bars") as e:
        check(err, bars, yard)
    print(net, case, mutant, str(e.value).split("\n")[0], "of", len(err))
    assert "yardstick" in str(e.value) and "bar" in str(e.value)
