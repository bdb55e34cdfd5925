"""The parity-bar rule, once, for every network (the networks' steps and runners: tests/parity_util.py).

A step is a dict of named float64 arrays - `y`, `loss`, `grad:<name>`, running statistics, ... - from the HIP path, from the
oracle in fp32 or from the oracle in fp64.  `errors` compares two of them.  The yardstick of a tensor is what the oracle
evaluated in fp32 deviates from the oracle evaluated in fp64 (the largest of three inputs, the parameters unchanged): the
oracle's error, never the kernels'.  The bar is K times the larger of that and the median of its group (the gradients, and
everything else), never above the flat bar the case had before."""
import math
from collections import OrderedDict
from contextlib import contextmanager

import numpy as np
import torch
import torch.nn.functional as F

FWD_TOL, GRAD_TOL = 1e-5, 1e-4          # the flat bars: forward (north-star bar: 1e-3), gradients; relative L2 against fp64
STEM_MARGIN = 1e-5          # the smallest distance from a kink a case with per-tensor bars may have (about 100 roundings of an O(1) sum)
# K = 8: the design lets an fp16-pair product be 2^-21 relative where fp32 rounds at 2^-24 (csrc/ral_device.hpp, DESIGN.md
# section 4), so a tensor may carry 2^3 times the error of an fp32 evaluation and no more
K_PAIR = 8.0
# K = 4 where no kernel multiplies fp16 pairs: the factor test_unet_bench_batch_matches_fp64_oracle allows over the fp32 oracle
K_FP32 = 4.0


def rel(a, b):
    a = np.asarray(a, dtype=np.float64).ravel(); b = np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def is_zero(ref):
    return float(np.linalg.norm(ref)) <= 1e-12


def errors(mine, ref):
    """{key: error} of the values `mine` against the fp64 values `ref`, in ref's order: relative L2 (of a scalar such as the
    loss: its relative difference); a `grad:` key whose fp64 value is zero (norm <= 1e-12) and every `gradabs:` key (a gradient
    that is identically zero, such as the key half of `to_kv.bias`: softmax shift invariance) as the largest |element|"""
    assert set(mine) == set(ref), sorted(set(mine) ^ set(ref))
    res = OrderedDict()
    for k, r in ref.items():
        m = np.asarray(mine[k], dtype=np.float64)
        assert m.size == r.size, (k, m.shape, r.shape)
        if k.startswith("gradabs:") or (k.startswith("grad:") and is_zero(r)):
            res[k] = float(np.abs(m).max())
        else:
            res[k] = rel(m, r)
    return res


# ------------------------------------------------------------------------------------------------------------------- kinks
class Kinks:
    """Stand-ins for the kinked functions of an oracle forward.  Each call notes which side every element took (`sides`, one
    (kind, tensor) per call, in call order) and keeps the smallest distance from a kink over the RMS of that call's tensor
    (`margin`, with `where`: kind and call number)."""

    def __init__(self):
        self.sides, self.margin, self.where, self.count = [], math.inf, None, 0

    def _note(self, kind, side, dist, t):
        m = dist.min().item() / t.detach().double().pow(2).mean().sqrt().item()
        if m < self.margin:
            self.margin, self.where = m, "%s, call %d" % (kind, len(self.sides))
        self.sides.append((kind, side))
        self.count += dist.numel()

    def leaky_relu(self, x, slope=0.01):
        self._note("leaky_relu", x.detach() > 0, x.detach().abs(), x)
        return F.leaky_relu(x, slope)

    def relu(self, x):
        self._note("relu", x.detach() > 0, x.detach().abs(), x)
        return torch.relu(x)

    def clamp(self, x, min=None, max=None):
        assert (min, max) in ((0, None), (None, 0))
        self._note("clamp", x.detach() > 0, x.detach().abs(), x)
        return torch.clamp(x, min=min, max=max)

    def max_pool1d(self, x, k):
        assert k == 2 and x.shape[-1] % 2 == 0
        a, b = x.detach()[..., 0::2], x.detach()[..., 1::2]
        self._note("max_pool1d", a >= b, (a - b).abs(), x)
        return F.max_pool1d(x, k)

    def adaptive_max_pool1d(self, x, n):
        assert n == 1
        top = x.detach().topk(2, -1)
        self._note("adaptive_max_pool1d", top.indices[..., 0], top.values[..., 0] - top.values[..., 1], x)
        return F.adaptive_max_pool1d(x, n)

    def same_sides(self, other):
        return len(self.sides) == len(other.sides) and all(
            ka == kb and torch.equal(a, b) for (ka, a), (kb, b) in zip(self.sides, other.sides))


class _Functional:
    """the functional namespace `base` with `over` on top"""
    def __init__(self, base, over):
        self._base = base
        self.__dict__.update(over)

    def __getattr__(self, name):
        return getattr(self._base, name)


@contextmanager
def standing_in(mod, F=None, **attrs):
    """Oracle module `mod` (ralenet_oracle, danet_oracle) with its module-level functions `attrs` replaced, and the entries
    `F` ({name: function}) of its `F`, torch.nn.functional; everything is put back on exit.  Nests: an inner context builds on
    what it finds and restores just that."""
    if F:
        attrs["F"] = _Functional(mod.F, F)
    keep = {k: getattr(mod, k) for k in attrs}
    for k, v in attrs.items():
        setattr(mod, k, v)
    try:
        yield
    finally:
        for k, v in keep.items():
            setattr(mod, k, v)


@contextmanager
def recording(mod):
    """oracle module `mod` with every kinked function recorded -> the Kinks"""
    k = Kinks()
    own = dict(relu=k.relu, clamp=k.clamp) if hasattr(mod, "clamp") else {}          # danet_oracle's module-level ones
    with standing_in(mod, F=dict(leaky_relu=k.leaky_relu, max_pool1d=k.max_pool1d, adaptive_max_pool1d=k.adaptive_max_pool1d), **own):
        yield k


def kink_precondition(step, seed, own, margin=None):
    """An fp32 evaluation that takes another branch of a kink than the fp64 one differs from it by a discrete amount that says
    nothing about rounding.  So, of `step(dtype, seed)` -> namespace with `kinks`: on the case's own input the fp64 evaluation
    keeps STEM_MARGIN from every kink - `margin()`, or the recorded distance over the RMS of its tensor - and on every input of
    the yardstick fp32 and fp64 take the same side of every kink and the same pool winners."""
    o = step(torch.float64, seed)
    if own:
        m = o.kinks.margin if margin is None else margin()
        assert m >= STEM_MARGIN, (seed, m, o.kinks.where)
    assert step(torch.float32, seed).kinks.same_sides(o.kinks), seed


# --------------------------------------------------------------------------------------------------------- yardstick, bars
def yardstick(step, seeds, precondition=kink_precondition):
    """What fp32 arithmetic itself costs, per key of `step(dtype, seed).vals`: errors(fp32 oracle, fp64 oracle) on the same
    seeded parameters and inputs.  `gradabs:` keys and gradients whose fp64 value is zero get None: a quantity whose true value
    is zero has no relative yardstick, and keeps its flat absolute bar.

    One fp32 evaluation is a single sample of each tensor's rounding error, and torch's summation order follows the thread
    count: the three-element `leconv.partial_conv3.weight` gradients of RA-LENet came out between 1.1e-7 and 5.5e-7 for the same
    case at 16 threads and at 1, the nearly cancelling attention query gradients of the spread cases vary fivefold from one
    input to the next - and the strict f16_split = 0 path, whose summation order is its own, sat 8.5 to 8.6 times above such a
    sample.  So the yardstick is the largest of three fp32 evaluations, each against its own fp64 one, on inputs from the three
    `seeds`, the case's own first; the parameters stay.  `bars` floors it at its group's median besides.

    `precondition(step, seed, own)` asserts what the case owes on each input (kink_precondition)."""
    assert len(seeds) == 3
    yard = None
    for s in seeds:
        precondition(step, s, s == seeds[0])
        e = errors(step(torch.float32, s).vals, step(torch.float64, s).vals)
        yard = e if yard is None else OrderedDict((k, max(v, e[k])) for k, v in yard.items())
    ref = step(torch.float64, seeds[0]).vals
    for k in yard:
        if k.startswith("gradabs:") or (k.startswith("grad:") and is_zero(ref[k])):
            yard[k] = None
    return yard


def _group(key):
    return 1 if key.startswith("grad:") else 0


def yardstick_floors(yard):
    """-> (median of the non-None yardsticks of the forward group, of the gradient group)"""
    return tuple(float(np.median([v for k, v in yard.items() if v is not None and _group(k) == g])) for g in (0, 1))


def bars(yard, K=K_PAIR, flat=(FWD_TOL, GRAD_TOL), capped=True, zero_abs=None, families=()):
    """One bar per key of `yard`: min(flat bar of the key's group, K * max(yard[key], median of yard over the group)); the
    groups are the gradients (`grad:*`, flat[1]) and everything else (flat[0]).  A key without a yardstick (None) has the
    absolute bar `zero_abs`, or the flat bar of its group.  A key that contains a string of `families` ((substring, K), ...)
    has that K, above `K` and at most K_PAIR, the project's largest.

    The median floor: the smallest single samples (4.5e-8 .. 1e-7, at small tensors) say little about the tensor's typical
    rounding error.  The min keeps every bar at or below the flat one; `capped=False` drops it, for cases whose tensors are ill
    conditioned in fp32 itself (the yardstick of such a tensor is above the flat bar, and so is what any fp32 kernel can reach)."""
    floors = yardstick_floors(yard)
    out = OrderedDict()
    for k, v in yard.items():
        g = _group(k)
        if v is None:
            out[k] = flat[g] if zero_abs is None else zero_abs
            continue
        Kk = K
        for sub, Kf in families:
            assert K < Kf <= K_PAIR
            if sub in k:
                Kk = Kf
        out[k] = Kk * max(v, floors[g])
        if capped:
            out[k] = min(flat[g], out[k])
    return out


def flat_bars(ref, flat=(FWD_TOL, GRAD_TOL), zero_abs=None):
    """the bars every case had before, per key of the fp64 values `ref`: flat[0], for a gradient flat[1]; for a gradient
    whose fp64 value is zero `zero_abs` (absolute), if given"""
    return OrderedDict((k, zero_abs if zero_abs is not None and k.startswith("grad:") and is_zero(r) else flat[_group(k)])
                       for k, r in ref.items())


def ratios(res, yard):
    """-> per group (forward, gradients): (worst error over yardstick, its key, median error over yardstick), the yardstick of a
    key being max(yard[key], median of yard over the group), as in `bars`; keys without a yardstick are left out"""
    floors = yardstick_floors(yard)
    out = []
    for g in (0, 1):
        r = {k: res[k] / max(y, floors[g]) for k, y in yard.items() if y is not None and k.startswith("grad:") == bool(g)}
        worst = max(r, key=r.get)
        out.append((r[worst], worst, float(np.median(list(r.values())))))
    return out


def check(res, bars, yard=None, what=""):
    """every error at or below its bar; a failure names the tensor, its error, its yardstick and its bar.  With the yardstick
    the bars came from: a line of what was observed."""
    assert list(res) == list(bars), sorted(set(res) ^ set(bars))
    if yard is not None:
        (fw, fk, fm), (gw, gk, gm) = ratios(res, yard)
        print(f"\nobserved {what}: error over yardstick: forward worst {fw:.2f} ({fk}) median {fm:.2f}, "
              f"gradient worst {gw:.2f} ({gk}) median {gm:.2f}")
    bad = {k: v for k, v in res.items() if not v <= bars[k]}
    yd = {k: "none" if yard is None or yard[k] is None else "%.3e" % yard[k] for k in bad}
    assert not bad, "\n".join(["%d tensors above their bars:" % len(bad)] + [
        f"  {k}: error {v:.3e}, yardstick {yd[k]}, bar {bars[k]:.3e}" for k, v in bad.items()])
