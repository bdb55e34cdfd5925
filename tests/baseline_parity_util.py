"""Per-tensor parity bars for the three baseline networks (U-Net, ACDAE, DANet) and the 12-lead adapter, by the rule of
parity_util.parity_yardstick / parity_bars: the yardstick of a tensor is what the oracle evaluated in fp32 deviates from the
oracle evaluated in fp64 (the largest of three inputs, the parameters unchanged), the bar K times the larger of that and the
median of its group, never above the flat bar the case had before.

A case is (network, shape, input seed):
  "unet"     (leads, L, B)     parameters O.init_params(..., 1234), inputs torch.Generator(seed): x, target
  "acdae"    (L, B)            the same
  "danet"    (B, L, leads)     state D.init_state(99), inputs torch.Generator(seed) - the GPU test's seed is B
  "newrale"  (variant, L, B)   parity_util.make_newrale_case

The kink precondition.  These networks are full of kinks: LeakyReLU(0.01) after every U-Net and ACDAE layer (one flipped sign
changes a gradient term a hundredfold), MaxPool1d(2) in ACDAE, in DANet the APReLU clamps, the ReLUs of the descriptor nets and
the DAM's two AdaptiveMaxPool1d.  An fp32 evaluation that takes another branch than the fp64 one differs from it by a discrete
amount that says nothing about rounding (DANet 64 x 512 at input seed 1064: 6.5e-3 median gradient error fp32 against fp64), and
a kernel may differ from both.  So the oracle runs with every kink recorded (Kinks), and a case gets per-tensor bars only if
  a. the smallest |pre-activation| is >= STEM_MARGIN x the RMS of its tensor,
  b. every max-pool winner is that far (x the RMS of the pool's input) ahead of the runner-up,
  c. the fp32 and the fp64 evaluation take the same side of every kink and the same pool winners, on all three inputs.
With n kink inputs a case fails (a) with probability about 1 - exp(-0.8e-5 n): the cases of 100 000 inputs and more find no
seed and keep their flat bars (CASES below holds what was found; tests/test_baseline_bars_cpu.py checks it)."""
import functools
import math
from collections import OrderedDict
from contextlib import contextmanager, nullcontext
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import danet_oracle as D
import ralenet_oracle as O
from parity_util import STEM_MARGIN, make_newrale_case, parity_bars, rel, yardstick_floors
from tie_util import oracle_functional

K_BASE = 4.0          # the factor test_unet_bench_batch_matches_fp64_oracle allows over the fp32 oracle; no fp16 pairs here
K_MAX = 8.0           # the project's largest (parity_util.parity_bars)
FWD_TOL, GRAD_TOL = 1e-5, 1e-4
DANET_ZERO = (".fcn.0.bias", ".fcn.3.bias", ".fcn1.0.bias", ".fcn1.3.bias")      # biases in front of a batch-statistics BatchNorm


# ------------------------------------------------------------------------------------------------------- recording kinks
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


@contextmanager
def recording(mod):
    """oracle module `mod` with every kinked function recorded -> the Kinks.  The convolutions stay torch's own, as in the
    GPU tests' references (tie_util.oracle_functional would put its tap-by-tap ones in)."""
    k = Kinks()
    over = dict(conv1d=F.conv1d, conv_transpose1d=F.conv_transpose1d, leaky_relu=k.leaky_relu, max_pool1d=k.max_pool1d,
                adaptive_max_pool1d=k.adaptive_max_pool1d)
    keep = (D.relu, D.clamp)
    if mod is D:
        D.relu, D.clamp = k.relu, k.clamp
    try:
        with oracle_functional(mod, **over):
            yield k
    finally:
        D.relu, D.clamp = keep


# ---------------------------------------------------------------------------------------------- defects for the fp32 oracle
# Each is a context manager entered inside recording(): it changes the module's functional (gone with the context) or a
# module-level function (restored here).  tests/test_baseline_bars_cpu.py holds what each does to the errors.
@contextmanager
def _bn_eps_unet():
    """BatchNorm eps 1.02e-5 where 1e-5 is specified (2e-5 is above the flat bars as well: channels of small variance)"""
    O.F.batch_norm = lambda t, rm, rv, w, b, tr, mom, eps: F.batch_norm(t, rm, rv, w, b, tr, mom, 1.02e-5)
    yield


@contextmanager
def _bn_eps_danet():
    """BatchNorm eps 1.0015e-5 (the descriptor nets normalise over the batch: a variance of B samples)"""
    keep = D._bn
    D._bn = lambda x, st, pre, training: keep(x, st, pre, training, eps=1.0015e-5)
    try:
        yield
    finally:
        D._bn = keep


@contextmanager
def _sigmoid_danet():
    """every gate of DANet (APReLU alpha, the DAM's channel and spatial attention) from a sigmoid that is 3e-6 relative too
    large: what an approximate exponential may cost"""
    keep = D.sigmoid
    D.sigmoid = lambda x: keep(x) * (1.0 + 3e-6)
    try:
        yield
    finally:
        D.sigmoid = keep


def _tap_scaled(taps, by):
    @contextmanager
    def mutant():
        """the middle tap of every `taps`-tap convolution times 1 + `by`"""
        def conv1d(x, w, *a, **k):
            if w.shape[-1] == taps:
                w = w * (1.0 + by * (torch.arange(taps) == taps // 2)).to(w.dtype)
            return F.conv1d(x, w, *a, **k)
        O.F.conv1d = conv1d
        yield
    return mutant


@contextmanager
def _upsample_weights():
    """the 0.25 / 0.75 weights of ACDAE's linear upsample 0.249999 / 0.750001: (1 - d) * linear + d * nearest with d = 4e-6
    (the nearest-neighbour upsample is the nearer of the two samples)"""
    def interpolate(x, **k):
        out = F.interpolate(x, **k)
        return out + 4e-6 * (F.interpolate(x, scale_factor=2, mode="nearest") - out)
    O.F.interpolate = interpolate
    yield


@contextmanager
def _stem_slope():
    """the stem's LeakyReLU(0.2) with slope 0.2 + 1e-5"""
    keep = O.F.leaky_relu
    O.F.leaky_relu = lambda x, s=0.01: keep(x, s + 1e-5 if s == 0.2 else s)
    yield


MUTANTS = {"unet_bn_eps": _bn_eps_unet, "danet_bn_eps": _bn_eps_danet, "danet_sigmoid": _sigmoid_danet, "acdae_tap13": _tap_scaled(13, 1e-5),
           "acdae_upsample": _upsample_weights, "newrale_tap13": _tap_scaled(13, 1e-5), "newrale_stem_slope": _stem_slope}


# ------------------------------------------------------------------------------------------------------------ oracle steps
def _inputs(B, leads, L, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, leads, L, generator=g), torch.randn(B, leads, L, generator=g)


def _np(t):
    return t.detach().double().numpy()


def _unet_step(case, dtype, seed):
    leads, L, B = case
    p32 = O.init_params(O.unet_param_shapes(leads), 1234)
    x, tgt = _inputs(B, leads, L, seed)
    p = OrderedDict((k, v.to(dtype).requires_grad_(True)) for k, v in p32.items())
    bn = O.unet_bn_state(p, dtype)
    y = O.unet_forward(p, x.to(dtype), True, bn)
    loss = O.mse(y, tgt.to(dtype))
    grads = torch.autograd.grad(loss, list(p.values()))
    with torch.no_grad():
        ye = O.unet_forward(OrderedDict((k, v.detach()) for k, v in p.items()), x.to(dtype), False, bn)
    v = OrderedDict(y=_np(y), loss=_np(loss))
    for k in O.UNET_BN:
        v[k + ".running_mean"], v[k + ".running_var"] = _np(bn[k]["running_mean"]), _np(bn[k]["running_var"])
    v.update(("grad:" + k, _np(g)) for k, g in zip(p, grads))
    v["y_eval"] = _np(ye)
    return v


def _acdae_step(case, dtype, seed):
    L, B = case
    p32 = O.init_params(O.acdae_param_shapes(), 1234)
    x, tgt = _inputs(B, 2, L, seed)
    p = OrderedDict((k, v.to(dtype).requires_grad_(True)) for k, v in p32.items())
    xd = x.to(dtype).requires_grad_(True)
    t = tgt.to(dtype)
    y = O.acdae_forward(p, xd)
    loss = O.mse(y, t)
    grads = torch.autograd.grad(loss, list(p.values()) + [xd])
    v = OrderedDict(y=_np(y), loss=_np(loss))
    v.update(("grad:" + k, _np(g)) for k, g in zip(p, grads))
    v["grad:input"] = _np(grads[-1])
    return v


def danet_states(leads):
    """(fp64 state, its fp32 copy) as the GPU test loads them: D.init_state(99) drawn in fp64"""
    st64 = D.init_state(99, leads=leads, dtype=torch.float64)
    for k in st64:
        if ".dam.fcn2." in k:
            assert st64[k] is st64[k.replace(".dam.fcn2.", ".dam.fcn1.")]
    st32 = OrderedDict()
    for k, v in st64.items():
        src = k.replace(".dam.fcn2.", ".dam.fcn1.")
        st32[k] = st32[src] if src != k else (v.clone().float() if v.dtype.is_floating_point else v.clone())
    return st64, st32


def danet_param_names(st):
    return [k for k in st if D.is_param(k) and ".dam.fcn2." not in k]


def danet_stat_names(st):
    return [k for k in st if k.endswith(("running_mean", "running_var"))]


def _danet_step(case, dtype, seed):
    """the eval forward on the initial running statistics first, then the train step: the order of the GPU test"""
    B, L, leads = case
    st = danet_states(leads)[0 if dtype == torch.float64 else 1]
    x, tgt = _inputs(B, leads, L, seed)
    with torch.no_grad():
        ye = D.danet_forward(st, x.to(dtype), training=False)
    params = OrderedDict((k, st[k].requires_grad_(True)) for k in danet_param_names(st))
    xd = x.to(dtype).requires_grad_(True)
    y = D.danet_forward(st, xd, training=True)
    loss = F.mse_loss(y, tgt.to(dtype))
    grads = torch.autograd.grad(loss, list(params.values()) + [xd])
    return danet_vals(ye, y, loss, grads[-1], OrderedDict(zip(params, grads)), st)


def danet_vals(ye, y, loss, dx, grads, st):
    """the quantities of one DANet step under their keys: `grads` {parameter name: gradient} in danet_param_names' order, `st`
    the state after the step"""
    v = OrderedDict(y_eval=_np(ye), y=_np(y), loss=_np(loss))
    v["grad:input"] = _np(dx)
    v.update(("grad:" + k, _np(grads[k])) for k in danet_param_names(st))
    v.update((k, _np(st[k])) for k in danet_stat_names(st))
    return v


def _newrale_step(case, dtype, seed):
    variant, L, B = case
    p32, pa32, x, tgt = make_newrale_case(variant, L, B, seed)
    p = OrderedDict((k, v.to(dtype)) for k, v in p32.items())
    pa = OrderedDict((k, v.to(dtype).requires_grad_(True)) for k, v in pa32.items())
    bn = O.new_bn_state(8, dtype)
    t = tgt.to(dtype)
    y = O.newrale_forward(pa, p, x.to(dtype), variant, True, bn)
    loss = O.mse(y, t)
    grads = torch.autograd.grad(loss, list(pa.values()))
    with torch.no_grad():
        ye = O.newrale_forward(OrderedDict((k, v.detach()) for k, v in pa.items()), p, x.to(dtype), variant, False, bn)
    v = OrderedDict(y=_np(y), loss=_np(loss), snr=_np(O.snr(t, y.detach())), rmse=_np(O.rmse(t, y.detach())))
    v.update(("grad:" + k, _np(g)) for k, g in zip(pa, grads))
    v["bn_mean"], v["bn_var"], v["y_eval"] = _np(bn["running_mean"]), _np(bn["running_var"]), _np(ye)
    return v


_STEPS = {"unet": (_unet_step, O), "acdae": (_acdae_step, O), "danet": (_danet_step, D), "newrale": (_newrale_step, O)}


@functools.lru_cache(maxsize=16)
def oracle_step(net, case, dtype, seed, mutant=None):
    """One train step and the eval forward that goes with it in the oracle alone, in `dtype`, on the seeded parameters of
    `net` and the inputs of `seed`; `mutant` names one of MUTANTS.  -> namespace: vals, one float64 numpy array per quantity
    the GPU test of `net` compares (`y`, `loss`, `grad:<name>`, running statistics, ...); kinks, the Kinks of the run.  Cached
    like parity_util._oracle_step and read-only for every caller."""
    fn, mod = _STEPS[net]
    with recording(mod) as kinks, (MUTANTS[mutant]() if mutant else nullcontext()):
        vals = fn(case, dtype, seed)
    return SimpleNamespace(vals=vals, kinks=kinks)


# ------------------------------------------------------------------------------------------------------ errors, yardstick
def is_zero(ref):
    return float(np.linalg.norm(ref)) <= 1e-12


def errors(mine, ref):
    """{key: error} of `mine` against the fp64 values `ref` (both as oracle_step's vals, `mine` in ref's order): relative L2;
    the loss as a relative difference; a gradient whose fp64 value is zero (norm <= 1e-12) as the largest |element|"""
    assert set(mine) == set(ref), sorted(set(mine) ^ set(ref))
    res = OrderedDict()
    for k, r in ref.items():
        m = np.asarray(mine[k], dtype=np.float64)
        assert m.size == r.size, (k, m.shape, r.shape)
        if k.startswith("grad:") and is_zero(r):
            res[k] = float(np.abs(m).max())
        else:
            res[k] = rel(m, r)
    return res


def oracle_errors(net, case, seed, mutant=None):
    """errors() with the fp32 oracle in the place of the HIP path; `mutant` changes the fp32 evaluation only"""
    return errors(oracle_step(net, case, torch.float32, seed, mutant).vals, oracle_step(net, case, torch.float64, seed).vals)


def kink_margin(net, case, seed):
    """-> (smallest distance from a kink over the RMS of its tensor, where) of the fp64 evaluation: conditions a and b"""
    k = oracle_step(net, case, torch.float64, seed).kinks
    return k.margin, k.where


def same_branches(net, case, seed):
    """condition c on one input"""
    return oracle_step(net, case, torch.float32, seed).kinks.same_sides(oracle_step(net, case, torch.float64, seed).kinks)


def precondition(net, case, seeds):
    """the kink precondition of a case whose own input is seeds[0] and whose yardstick uses all of `seeds`"""
    return kink_margin(net, case, seeds[0])[0] >= STEM_MARGIN and all(same_branches(net, case, s) for s in seeds)


def yardstick(net, case, seeds):
    """What fp32 arithmetic itself costs, per key of oracle_step(net, case, ...).vals: the largest of len(seeds) fp32-against-
    fp64 evaluations (parity_util.parity_yardstick's rule); None for a gradient whose fp64 value is zero.  Asserts the kink
    precondition."""
    assert len(seeds) == 3
    margin, where = kink_margin(net, case, seeds[0])
    assert margin >= STEM_MARGIN, (net, case, seeds[0], margin, where)
    yard = None
    for s in seeds:
        assert same_branches(net, case, s), (net, case, s)
        e = oracle_errors(net, case, s)
        yard = e if yard is None else OrderedDict((k, max(v, e[k])) for k, v in yard.items())
    ref = oracle_step(net, case, torch.float64, seeds[0]).vals
    for k in yard:
        if k.startswith("grad:") and is_zero(ref[k]):
            yard[k] = None
    return yard


def flat_bars(ref, flat=(FWD_TOL, GRAD_TOL), zero_abs=1e-5):
    """the bars every case had before, per key of the fp64 values `ref`: flat[0], for a gradient flat[1], and `zero_abs`
    (absolute) for a gradient whose fp64 value is zero"""
    return OrderedDict((k, flat[0] if not k.startswith("grad:") else zero_abs if is_zero(r) else flat[1]) for k, r in ref.items())


def bars_of(yard, flat=(FWD_TOL, GRAD_TOL), zero_abs=1e-5, families=()):
    """parity_bars(yard, K_BASE, flat) - capped at the flat bars the case had - with the absolute bar `zero_abs` for the keys
    without a yardstick, and for the keys that contain a string of `families` ((substring, K), ...) that K, at most K_MAX"""
    bars = parity_bars(yard, K_BASE, flat)
    for sub, K in families:
        assert K_BASE < K <= K_MAX
        wide = parity_bars(yard, K, flat)
        bars.update((k, wide[k]) for k in bars if sub in k)
    bars.update((k, zero_abs) for k, v in yard.items() if v is None)
    return bars


def ratios(res, yard):
    """test_gpu_parity.yardstick_ratios: per group (forward, gradients) (worst error over yardstick, its key, the median)"""
    floors = yardstick_floors(yard)
    out = []
    for g in (0, 1):
        r = {k: res[k] / max(y, floors[g]) for k, y in yard.items() if y is not None and k.startswith("grad:") == bool(g)}
        worst = max(r, key=r.get)
        out.append((r[worst], worst, float(np.median(list(r.values())))))
    return out


def check(res, bars, yard=None, what=""):
    """every error at or below its bar; a failure names the tensor, its error, its yardstick and its bar"""
    assert list(res) == list(bars), sorted(set(res) ^ set(bars))
    if yard is not None:
        (fw, fk, fm), (gw, gk, gm) = ratios(res, yard)
        print(f"\nobserved {what}: error over yardstick: forward worst {fw:.2f} ({fk}) median {fm:.2f}, "
              f"gradient worst {gw:.2f} ({gk}) median {gm:.2f}")
    bad = {k: v for k, v in res.items() if not v <= bars[k]}
    yd = {k: "none" if yard is None or yard[k] is None else "%.3e" % yard[k] for k in bad}
    assert not bad, "\n".join(["%d tensors above their bars:" % len(bad)] + [
        f"  {k}: error {v:.3e}, yardstick {yd[k]}, bar {bars[k]:.3e}" for k, v in bad.items()])


# ------------------------------------------------------------------------------------------------------------------ cases
# (case, input seed, the three input seeds of its yardstick - its own first - or None: flat bars).  A case whose own seed
# misses the precondition runs twice: at a seed that meets it with per-tensor bars, at the old one with the flat bars.
# Margins (smallest distance from a kink over the RMS, fp64) in the comments; STEM_MARGIN is 1e-5.
CASES = {
    "unet": [
        ((2, 512, 4), 2023, (2023, 2024, 2025)),        # 4.4e-5
        ((1, 256, 3), 2023, (2023, 2024, 2025)),        # 4.6e-5
        ((2, 1024, 2), 2023, (2023, 2024, 2025)),       # 1.6e-5
        ((2, 48, 5), 2024, (2024, 2025, 2026)),         # 2.7e-4
        ((2, 48, 5), 2023, None),                       # 2.4e-6
        ((2, 320, 3), 2023, (2023, 2024, 2025)),        # 1.2e-4
        ((2, 64, 1025), 2023, None),                    # 2.4 M kink inputs: 6.0e-7, and 2.9e-8 .. 1.8e-6 at seeds 2024 .. 2031
    ],
    "acdae": [
        ((512, 4), 2025, (2025, 2023, 2024)),           # 2.8e-5
        ((512, 4), 2023, None),                         # 9.0e-6
        ((256, 3), 2023, (2023, 2024, 2025)),           # 4.2e-5
        ((1024, 2), 2026, (2026, 2023, 2024)),          # 1.3e-5
        ((1024, 2), 2023, None),                        # 4.9e-6
        ((64, 3), 2023, (2023, 2024, 2025)),            # 6.6e-5
        ((192, 2), 2023, (2023, 2024, 2025)),           # 6.6e-5
    ],
    # (B, L, leads); the old tests' input seed is B.  The three large cases have 0.6 .. 2.2 M kink inputs and found no seed
    # among nine (own .. own + 8: 5.4e-8 .. 6.7e-6).  (8, 512, 2), (4, 1024, 2) and (8, 256, 2) are new: the long windows at batches
    # small enough (140 000 .. 280 000 kink inputs) for one seed in five to fifteen to meet the precondition; of those that do, one
    # at which the fp32 oracle also stays on the fp64 trajectory through the three Adam steps that follow (8, 512, 2: seed 20)
    "danet": [
        ((64, 512, 2), 64, None),                       # 7.2e-7
        ((37, 256, 2), 37, None),                       # 3.0e-6
        ((16, 1024, 2), 16, None),                      # 3.5e-6
        ((8, 512, 2), 20, (20, 21, 22)),                # 1.7e-5
        ((4, 1024, 2), 8, (8, 9, 10)),                  # 1.2e-5
        ((8, 256, 2), 8, (8, 9, 10)),                   # 2.6e-5
        ((8, 32, 2), 10, (10, 11, 12)),                 # 5.0e-5 (seed 9, 1.1e-4, is no case for the three Adam steps that
                                                        # follow: the fp32 oracle itself leaves the fp64 trajectory there, 1.4e-4)
        ((8, 32, 2), 8, None),                          # 3.8e-6
        ((4, 64, 2), 4, (4, 5, 6)),                     # 4.9e-5
    ],
    "newrale": [
        (("full", 256, 3), 2023, (2023, 2024, 2025)),   # 4.2e-5
        (("nra", 16, 4), 2023, (2023, 2024, 2025)),     # 1.9e-3
        (("full", 32, 2), 2023, (2023, 2024, 2025)),    # 8.8e-4
        (("mlp", 320, 2), 2023, (2023, 2024, 2025)),    # 5.2e-5
        (("nra", 64, 5), 2024, (2024, 2025, 2026)),     # 4.3e-4
        (("nra", 64, 5), 2023, None),                   # 8.2e-6
        (("full", 1008, 1), 2023, (2023, 2024, 2025)),  # 1.4e-5
        (("nra", 16, 513), 2023, None),                 # 361 000 kink inputs: 6.7e-6, and 2.2e-7 .. 9.8e-6 at seeds 2024 .. 2031
    ],
}


def own_seed(net, case):
    """the input seed the GPU tests always had: 2023, for DANet the batch size"""
    return case[0] if net == "danet" else 2023


def case_id(net, entry):
    """the shape, as the tests' ids always were; a case at another seed than own_seed says so"""
    case, seed, _ = entry
    return "-".join(str(c) for c in case) + ("" if seed == own_seed(net, case) else "-seed%d" % seed)


def case_params(net):
    import pytest
    return [pytest.param(*e, id=case_id(net, e)) for e in CASES[net]]


# Flat caps and absolute bars of zero gradients, as the GPU tests had them
def danet_gtol(case):
    """a BatchNorm over a batch of 4 descriptors divides by a variance of four samples: fp32 rounding is amplified there"""
    return 1e-4 if case[0] >= 8 else 2e-3


def caps(net, case):
    """-> ((forward cap, gradient cap), absolute bar of a zero gradient)"""
    if net == "danet":
        return (FWD_TOL, danet_gtol(case)), 1e-5
    return (FWD_TOL, GRAD_TOL), 2e-5 if net == "unet" else 1e-5


# Key families with a K of their own: (network, substring of the key, K, why).  Empty unless a healthy tensor measured
# above K_BASE on the GPU for a reason of summation order.
FAMILIES = ()


def case_bars(net, case, seed, seeds):
    """-> (bars, yardstick or None) of one entry of CASES"""
    flat, zero_abs = caps(net, case)
    if seeds is None:
        ref = oracle_step(net, case, torch.float64, seed).vals if net != "danet" else None
        return (flat_bars(ref, flat, zero_abs) if ref is not None else None), None
    assert seeds[0] == seed
    yard = yardstick(net, case, seeds)
    return bars_of(yard, flat, zero_abs, tuple((sub, K) for n, sub, K, _ in FAMILIES if n == net)), yard


# ------------------------------------------------------------------------------------------------------- the HIP path
def run_unet(case, seed, device):
    """one train step and the eval forward after it on the HIP path -> (vals as oracle_step's, the model in eval mode)"""
    from ecg_denoise_amd import UNet
    leads, L, B = case
    p32 = O.init_params(O.unet_param_shapes(leads), 1234)
    x, tgt = _inputs(B, leads, L, seed)
    m = UNet(leads=leads, L=L, max_batch=B, device=device)
    m.load_state_dict(p32, strict=False)
    m.train()
    y = m(x.to(device))
    loss, _, _ = m.loss_and_metrics(y, tgt.to(device))
    m.backward()
    torch.cuda.synchronize()
    v = OrderedDict(y=_np(y.cpu()), loss=_np(loss.cpu()))
    sd = m.state_dict()
    for k in O.UNET_BN:
        v[k + ".running_mean"], v[k + ".running_var"] = _np(sd[k + ".running_mean"].cpu()), _np(sd[k + ".running_var"].cpu())
    ng = m.named_grads()
    v.update(("grad:" + k, _np(ng[k].cpu())) for k in p32)
    m.eval()
    v["y_eval"] = _np(m(x.to(device)).cpu())
    return v, m


def run_acdae(case, seed, device):
    """one train step on the HIP path -> (vals, the model, x, y, snr, target)"""
    from ecg_denoise_amd import ACDAE
    L, B = case
    p32 = O.init_params(O.acdae_param_shapes(), 1234)
    x, tgt = _inputs(B, 2, L, seed)
    m = ACDAE(L=L, max_batch=B, device=device)
    m.load_state_dict(p32)
    m.train()
    y = m(x.to(device))
    loss, snr, _ = m.loss_and_metrics(y, tgt.to(device))
    dx = m.backward(want_dx=True)
    torch.cuda.synchronize()
    v = OrderedDict(y=_np(y.cpu()), loss=_np(loss.cpu()))
    ng = m.named_grads()
    v.update(("grad:" + k, _np(ng[k].cpu())) for k in p32)
    v["grad:input"] = _np(dx.cpu())
    return v, m, x, y, snr, tgt
