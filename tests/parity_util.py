"""Shared helpers of the GPU parity tests: for each of the five networks one oracle step and one run of the HIP path on the same
seeded inputs, both as named float64 values under the keys the network's GPU test compares (the rule that turns them into errors,
yardsticks and bars: tests/parity_bars.py; the cases of the baselines and the adapter: tests/baseline_parity_util.py).

A case is (network, shape, input seed):
  "ralenet"  (variant, leads, L, B)   parameters O.init_params(..., 1234), inputs torch.Generator(seed): x, target (make_case)
  "unet"     (leads, L, B)            the same
  "acdae"    (L, B)                   the same
  "danet"    (B, L, leads)            state D.init_state(99), inputs torch.Generator(seed) - the GPU test's seed is B
  "newrale"  (variant, L, B)          make_newrale_case"""
import functools
import inspect
from collections import OrderedDict
from contextlib import nullcontext
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import danet_oracle as D
import ralenet_oracle as O
from parity_bars import errors, kink_precondition, recording, rel, standing_in, yardstick  # noqa: F401 (rel: fifteen files import it from here)

THREE_SEEDS = (2023, 2024, 2025)
STEM = ("conv1.0.", "conv1.2.")


def oracle_trace(p, x, variant, bn, dtype=torch.float64):
    """Oracle forward (training mode) that also returns every block / resample output,
    named like the library's debug tensors."""
    F = O.F          # (the oracle's own: a recorded or mutated functional reaches the stem here as well)
    le, rw, _ = O.variant_flags(variant)
    tr = OrderedDict()
    B, _, L = x.shape
    y = F.conv1d(x, p["conv1.0.weight"], p["conv1.0.bias"], padding=1)
    y = F.leaky_relu(y, 0.2)
    tr["a0"] = y.permute(0, 2, 1)
    y = F.batch_norm(y, bn["running_mean"], bn["running_var"], p["conv1.2.weight"], p["conv1.2.bias"], True, 0.1, 1e-5)
    x0 = y
    tr["x0"] = y.permute(0, 2, 1)
    biases = [None] * 5
    if rw:
        for i, ln in enumerate(O.RW_LEN):
            biases[i + 1] = O.rwave_bias(p[f"rwattn{i+1}.relative_position_bias_table"], ln, L >> i)
    bi = [0]

    def stage(t, name, rwi):
        for i in range(2):
            t = O.transformer_block(t, p, O.block_prefix(variant, name, i), le, biases[rwi] if rwi else None)
            tr[f"blk{bi[0]}.out"] = t
            bi[0] += 1
        return t

    t = y.permute(0, 2, 1)
    x1 = O.patch_merge(stage(t, "dtransformer1", 1), p, "pm1"); tr["p1"] = x1
    x2 = O.patch_merge(stage(x1, "dtransformer2", 2), p, "pm2"); tr["p2"] = x2
    x3 = O.patch_merge(stage(x2, "dtransformer3", 3), p, "pm3"); tr["p3"] = x3
    x4 = O.patch_merge(stage(x3, "dtransformer34", 4), p, "pm4"); tr["p4"] = x4
    xm = stage(x4, "transformer", 0) + x4; tr["xmid"] = xm
    d = O.patch_separate(stage(xm, "utransformer4", 0), p, "ps4") + x3; tr["u3"] = d
    d = O.patch_separate(stage(d, "utranformer3", 4), p, "ps3") + x2; tr["u2"] = d
    d = O.patch_separate(stage(d, "utransformer2", 3), p, "ps2") + x1; tr["u1"] = d
    d = O.patch_separate(stage(d, "utransformer1", 2), p, "ps1"); tr["u0"] = d
    d = d.permute(0, 2, 1) + x0
    out = F.conv1d(d, p["transconv.0.weight"], p["transconv.0.bias"], padding=1)
    return out, tr


def make_case(variant, leads, L, B, seed=1234, dtype=torch.float64, input_seed=2023):
    p32 = O.init_params(O.ralenet_param_shapes(variant, leads), seed)
    g = torch.Generator().manual_seed(input_seed)
    x = torch.randn(B, leads, L, generator=g)
    tgt = torch.randn(B, leads, L, generator=g)
    return p32, x, tgt


def make_newrale_case(variant, L, B, input_seed=2023):
    """`make_case`'s seeds for the 12-lead adapter: inner 2-lead RA-LENet parameters (1234), adapter parameters (77), x and
    target (B, 12, L) from generator `input_seed`"""
    p32 = O.init_params(O.ralenet_param_shapes(variant, 2), 1234)
    pa32 = O.init_params(O.newrale_param_shapes(), 77)
    g = torch.Generator().manual_seed(input_seed)
    x = torch.randn(B, 12, L, generator=g)
    tgt = torch.randn(B, 12, L, generator=g)
    return p32, pa32, x, tgt


def _inputs(B, leads, L, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, leads, L, generator=g), torch.randn(B, leads, L, generator=g)


def _np(t):
    return t.detach().cpu().double().numpy()


def grad_values(p, grads):
    """RA-LENet's parameter gradients `grads` (in the order of `p`, None where unused: zero) as values "grad:<name>".  The key
    half of a `to_kv.bias` gradient is identically zero (softmax shift invariance): the value half is "grad:<name>[v]", the key
    half "gradabs:<name>[k]", which `errors` bounds by rounding noise."""
    v = OrderedDict()
    for k, g in zip(p, grads):
        g = np.zeros(tuple(p[k].shape)) if g is None else _np(g)
        if k.endswith("to_kv.bias"):
            C = g.size // 2
            v["grad:" + k + "[v]"], v["gradabs:" + k + "[k]"] = g[C:], g[:C]
        else:
            v["grad:" + k] = g
    return v


def compare_grads(ng, p, grads):
    """error per parameter gradient (parity_bars.errors): the library's `named_grads()` against the oracle's `grads` (in the order of `p`)"""
    return errors(grad_values(p, [ng[k] for k in p]), grad_values(p, grads))


def stem_margin(variant, leads, L, B, seed=1234, params=None, input_seed=2023):
    """the smallest |stem pre-activation| of the case in fp64: its distance from the kink of the stem's LeakyReLU(0.2)"""
    p32, x, _ = make_case(variant, leads, L, B, seed, input_seed=input_seed)
    if params is not None:
        p32 = params(p32)
    return F.conv1d(x.double(), p32["conv1.0.weight"].double(), p32["conv1.0.bias"].double(), padding=1).abs().min().item()


def spread_fc1_bias(p32, lim=9.0, seed=5):
    """Every `*.mlp.fc1.bias` (H = 32 .. 512 hidden units) becomes torch.linspace(-lim, lim, H) in a seeded random order; the
    fc1 weights stay, so the GELU arguments are this grid plus each token's own fc1 output: dense over [-lim - 1, lim + 1], where
    the seeded parameters alone keep them below 3."""
    g = torch.Generator().manual_seed(seed)
    out = OrderedDict(p32)
    for k, v in p32.items():
        if k.endswith(".mlp.fc1.bias"):
            H = v.numel()
            out[k] = torch.linspace(-lim, lim, H, dtype=v.dtype)[torch.randperm(H, generator=g)]
    return out


# ------------------------------------------------------------------------------------------------------------ oracle steps
# One train step and the eval forward that goes with it in the oracle alone, in `dtype`: fn(case, dtype, seed, **options) ->
# dict(vals = one float64 array per quantity the network's GPU test compares, ...)
def _ralenet_step(case, dtype, seed, param_seed=1234, params=None, gelu=None):
    """`params`: a callable p32 -> p32 applied to the seeded parameters (spread_fc1_bias); `gelu` stands in for O.gelu (the
    mutants of tests/test_parity_bars_cpu.py).  `grad:input_frozen` and the `@dx` stem gradients repeat `grad:input` and the
    stem gradients: the oracle has one backward pass."""
    variant, leads, L, B = case
    p32, x, tgt = make_case(variant, leads, L, B, param_seed, input_seed=seed)
    if params is not None:
        p32 = params(p32)
    p = OrderedDict((k, v.to(dtype).requires_grad_(True)) for k, v in p32.items())
    bn = O.new_bn_state(8, dtype)
    xo = x.to(dtype).requires_grad_(True)          # (x is a leaf: the input gradient comes out of the same autograd call)
    t = tgt.to(dtype)
    with standing_in(O, gelu=gelu) if gelu is not None else nullcontext():
        yo, tr = oracle_trace(p, xo, variant, bn)
        lo = O.mse(yo, t)
        *grads, dxo = torch.autograd.grad(lo, list(p.values()) + [xo], allow_unused=True)
        with torch.no_grad():
            ye = O.ralenet_forward(OrderedDict((k, v.detach()) for k, v in p.items()), x.to(dtype), variant, training=False, bn=bn)
    yo = yo.detach()
    v = OrderedDict(y=_np(yo), loss=_np(lo), snr=_np(O.snr(t, yo)), rmse=_np(O.rmse(t, yo)),
                    bn_mean=_np(bn["running_mean"]), bn_var=_np(bn["running_var"]))
    v.update(("act:" + k, _np(a)) for k, a in tr.items())
    v.update(grad_values(p, grads))
    v["grad:input"] = _np(dxo)
    v.update(("grad:" + k + "@dx", v["grad:" + k]) for k in p if k.startswith(STEM))
    v["grad:input_frozen"] = v["grad:input"]
    v["y_eval"] = _np(ye)
    return dict(vals=v)


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
    return dict(vals=v)


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
    return dict(vals=v)


DANET_ZERO = (".fcn.0.bias", ".fcn.3.bias", ".fcn1.0.bias", ".fcn1.3.bias")      # biases in front of a batch-statistics BatchNorm


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
    """the eval forward on the initial running statistics first, then the train step: the order of the GPU test.  Besides
    vals: `state` after the step, `params` (its leaves, each with its gradient in .grad), `x` and `tgt` in `dtype` - from
    fresh_step they are live, for the Adam steps of tests/test_gpu_danet.py to go on from"""
    B, L, leads = case
    st = danet_states(leads)[0 if dtype == torch.float64 else 1]
    x, tgt = (t.to(dtype) for t in _inputs(B, leads, L, seed))
    with torch.no_grad():
        ye = D.danet_forward(st, x, training=False)
    params = OrderedDict((k, st[k].requires_grad_(True)) for k in danet_param_names(st))
    xd = x.clone().requires_grad_(True)
    y = D.danet_forward(st, xd, training=True)
    loss = F.mse_loss(y, tgt)
    *grads, dx = torch.autograd.grad(loss, list(params.values()) + [xd])
    v = OrderedDict(y_eval=_np(ye), y=_np(y), loss=_np(loss))
    v["grad:input"] = _np(dx)
    for (k, p), g in zip(params.items(), grads):
        v["grad:" + k], p.grad = _np(g), g
    v.update((k, _np(st[k])) for k in danet_stat_names(st))
    return dict(vals=v, state=st, params=params, x=x, tgt=tgt)


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
    return dict(vals=v)


STEPS = {"ralenet": (_ralenet_step, O), "unet": (_unet_step, O), "acdae": (_acdae_step, O), "danet": (_danet_step, D),
         "newrale": (_newrale_step, O)}


# ---------------------------------------------------------------------------------------------- defects for the fp32 oracle
# Each returns a context (parity_bars.standing_in) that builds on the oracle module as it finds it - recorded, inside step() -
# and puts back what it changed.  tests/test_baseline_bars_cpu.py holds what each does to the errors.
def _bn_eps_unet():
    """BatchNorm eps 1.02e-5 where 1e-5 is specified (2e-5 is above the flat bars as well: channels of small variance)"""
    return standing_in(O, F=dict(batch_norm=lambda t, rm, rv, w, b, tr, mom, eps: F.batch_norm(t, rm, rv, w, b, tr, mom, 1.02e-5)))


def _bn_eps_danet():
    """BatchNorm eps 1.0015e-5 (the descriptor nets normalise over the batch: a variance of B samples)"""
    keep = D._bn
    return standing_in(D, _bn=lambda x, st, pre, training: keep(x, st, pre, training, eps=1.0015e-5))


def _sigmoid_danet():
    """every gate of DANet (APReLU alpha, the DAM's channel and spatial attention) from a sigmoid that is 3e-6 relative too
    large: what an approximate exponential may cost"""
    keep = D.sigmoid
    return standing_in(D, sigmoid=lambda x: keep(x) * (1.0 + 3e-6))


def _tap_scaled(taps, by):
    def mutant():
        """the middle tap of every `taps`-tap convolution times 1 + `by`"""
        def conv1d(x, w, *a, **k):
            if w.shape[-1] == taps:
                w = w * (1.0 + by * (torch.arange(taps) == taps // 2)).to(w.dtype)
            return F.conv1d(x, w, *a, **k)
        return standing_in(O, F=dict(conv1d=conv1d))
    return mutant


def _upsample_weights():
    """the 0.25 / 0.75 weights of ACDAE's linear upsample 0.249999 / 0.750001: (1 - d) * linear + d * nearest with d = 4e-6
    (the nearest-neighbour upsample is the nearer of the two samples)"""
    def interpolate(x, **k):
        out = F.interpolate(x, **k)
        return out + 4e-6 * (F.interpolate(x, scale_factor=2, mode="nearest") - out)
    return standing_in(O, F=dict(interpolate=interpolate))


def _stem_slope():
    """the stem's LeakyReLU(0.2) with slope 0.2 + 1e-5"""
    keep = O.F.leaky_relu
    return standing_in(O, F=dict(leaky_relu=lambda x, s=0.01: keep(x, s + 1e-5 if s == 0.2 else s)))


MUTANTS = {"unet_bn_eps": _bn_eps_unet, "danet_bn_eps": _bn_eps_danet, "danet_sigmoid": _sigmoid_danet, "acdae_tap13": _tap_scaled(13, 1e-5),
           "acdae_upsample": _upsample_weights, "newrale_tap13": _tap_scaled(13, 1e-5), "newrale_stem_slope": _stem_slope}


def fresh_step(net, case, dtype, seed, mutant=None, **options):
    """The oracle step of `net` (STEPS) with every kink recorded; `mutant` names one of MUTANTS, `options` are the step's own
    (RA-LENet: param_seed, params, gelu).  -> namespace: vals; kinks, the Kinks of the run; what else the step hands back."""
    fn, mod = STEPS[net]
    with recording(mod) as kinks, (MUTANTS[mutant]() if mutant else nullcontext()):
        return SimpleNamespace(kinks=kinks, **fn(case, dtype, seed, **options))


@functools.lru_cache(maxsize=16)
def _cached_step(net, case, dtype, seed, mutant, options):
    return fresh_step(net, case, dtype, seed, mutant, **dict(options))


def step(net, case, dtype, seed, mutant=None, trace=True, eval_forward=True, **options):
    """fresh_step, cached: shared between a test's reference and its yardstick, and read-only for every caller.  Without
    `trace` the values leave out the `act:` keys, without `eval_forward` `y_eval`."""
    defaults = inspect.signature(STEPS[net][0]).parameters
    o = _cached_step(net, case, dtype, seed, mutant, tuple(sorted((k, v) for k, v in options.items() if v != defaults[k].default)))
    if trace and eval_forward:
        return o
    vals = OrderedDict((k, v) for k, v in o.vals.items() if (trace or not k.startswith("act:")) and (eval_forward or k != "y_eval"))
    return SimpleNamespace(**dict(vars(o), vals=vals))


def parity_yardstick(variant, leads, L, B, seed=1234, params=None, eval_forward=False, trace=True, input_seeds=THREE_SEEDS):
    """parity_bars.yardstick of an RA-LENet case, under the keys of run_parity(variant, leads, L, B, ...)'s result.
    Precondition: the stem's LeakyReLU(0.2) is the one kink of RA-LENet, and an fp32 pre-activation on the other side of 0
    from the fp64 one changes gradients by a discrete amount no yardstick describes - the smallest |stem pre-activation| of the
    case (fp64) must be >= STEM_MARGIN, absolute, and on all three inputs no fp32 pre-activation may change sides."""
    assert input_seeds[0] == 2023
    case = (variant, leads, L, B)
    return yardstick(lambda dtype, s: step("ralenet", case, dtype, s, None, trace, eval_forward, param_seed=seed, params=params), input_seeds,
                     functools.partial(kink_precondition, margin=lambda: stem_margin(variant, leads, L, B, seed, params)))


# ------------------------------------------------------------------------------------------------------- the HIP path
# run_<net>(case, seed, device) -> (the values of step(net, case, ...), from the library; the model; ...)
def run_ralenet(case, seed, device, trace=(), eval_forward=False, options=None, before_forward=None, params=None, param_seed=1234):
    """-> (vals, the model, (p32, x, tgt)).  `trace`: the names of the debug tensors to return as "act:<name>", each whole, laid
    out on the model's token slots.
    Gradients: every parameter gradient of `backward()` (dx = NULL, the training default); then "grad:input" and the stem
    parameter gradients "grad:<name>@dx" of `backward(want_dx=True)`, and "grad:input_frozen" of `backward_input` - the model
    comes back with the gradient buffer that last call left."""
    from ecg_denoise_amd import RALENet, _lib
    variant, leads, L, B = case
    p32, x, tgt = make_case(variant, leads, L, B, param_seed, input_seed=seed)
    if params is not None:
        p32 = params(p32)
    model = RALENet(variant, leads=leads, L=L, max_batch=B, train=True, device=device)
    model.load_state_dict(p32, strict=False)
    for key, value in (options or {}).items():
        _lib.check(_lib.lib().ral_set_option(model.eng.h, key.encode(), int(value)))
    if before_forward is not None:
        before_forward(model)
    xd, td = x.to(device), tgt.to(device)
    model.train()
    y = model(xd)
    loss, snr, rmse = model.loss_and_metrics(y, td)
    model.backward()
    torch.cuda.synchronize()
    st = model.state_dict()
    v = OrderedDict(y=_np(y), loss=_np(loss), snr=_np(snr), rmse=_np(rmse), bn_mean=_np(st["conv1.2.running_mean"]),
                    bn_var=_np(st["conv1.2.running_var"]))
    v.update(("act:" + k, _np(model.debug_tensor(k))) for k in trace)
    v.update(grad_values(p32, [model.named_grads()[k] for k in p32]))
    # the backward pass again on the same saved forward, now with the input gradient (ral_backward zeroes the gradient buffer
    # itself): the stem kernel that formed only parameter gradients above stores dz as well - its parameter gradients are compared
    # again, as grad:<name>@dx - and k_conv1_bwd_dx turns dz into dx
    dx = model.backward(want_dx=True)
    torch.cuda.synchronize()
    v["grad:input"] = _np(dx)
    v.update(("grad:" + k + "@dx", _np(model.named_grads()[k])) for k in p32 if k.startswith(STEM))
    # the frozen-weight chain (what NewRALE training runs: no weight-gradient kernels) from the same dy
    dxf = model.backward_input(model._dy)
    torch.cuda.synchronize()
    v["grad:input_frozen"] = _np(dxf)
    if eval_forward:
        model.eval()
        v["y_eval"] = _np(model(xd))
        model.train()
    return v, model, (p32, x, tgt)


def run_parity(variant, leads, L, B, device="cuda:0", trace=True, seed=1234, options=None, eval_forward=False, before_forward=None,
               params=None):
    """-> (dict of errors, HIP fp32 against the fp64 oracle - parity_bars.errors of run_ralenet against step("ralenet", ...) at
    input seed 2023; the model; (p32, x, tgt)).  `options`: {name: value} for ral_set_option on the model's handle, applied
    before the first forward.  `params`: a callable p32 -> p32 applied to the seeded parameters (of seed `seed`) before the
    model and the oracle see them (spread_fc1_bias).  `eval_forward`: after the train step, the eval-mode forward of the same
    model against the oracle's eval output (its BatchNorm on the running statistics the step left) as res["y_eval"].
    `before_forward(model)` is called once the options are set."""
    case = (variant, leads, L, B)
    ref = step("ralenet", case, torch.float64, 2023, None, trace, eval_forward, param_seed=seed, params=params).vals
    acts = [k[4:] for k in ref if k.startswith("act:")]
    mine, model, inputs = run_ralenet(case, 2023, device, acts, eval_forward, options, before_forward, params, seed)
    mine.update((k, mine[k].ravel()[:ref[k].size]) for k in ref if k.startswith("act:"))
    return errors(mine, ref), model, inputs


def run_unet(case, seed, device):
    """one train step and the eval forward after it -> (vals, the model in eval mode)"""
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
    v = OrderedDict(y=_np(y), loss=_np(loss))
    sd = m.state_dict()
    for k in O.UNET_BN:
        v[k + ".running_mean"], v[k + ".running_var"] = _np(sd[k + ".running_mean"]), _np(sd[k + ".running_var"])
    ng = m.named_grads()
    v.update(("grad:" + k, _np(ng[k])) for k in p32)
    m.eval()
    v["y_eval"] = _np(m(x.to(device)))
    return v, m


def run_acdae(case, seed, device):
    """one train step -> (vals, the model, x, y, snr, target)"""
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
    v = OrderedDict(y=_np(y), loss=_np(loss))
    ng = m.named_grads()
    v.update(("grad:" + k, _np(ng[k])) for k in p32)
    v["grad:input"] = _np(dx)
    return v, m, x, y, snr, tgt


def run_danet(case, seed, device):
    """the eval forward on the initial running statistics, then one train step -> (vals, the model in train mode, x and
    target on the device)"""
    from ecg_denoise_amd import DANet
    B, L, leads = case
    xd, td = (t.to(device) for t in _inputs(B, leads, L, seed))
    m = DANet(L=L, max_batch=B, train=True, device=device, leads=leads)
    m.load_state_dict(danet_states(leads)[1])
    m.eval()
    v = OrderedDict(y_eval=_np(m(xd)))
    m.train()
    y = m(xd)
    v["y"] = _np(y)
    loss, _, _ = m.loss_and_metrics(y, td)
    v["loss"] = _np(loss)
    v["grad:input"] = _np(m.backward(want_dx=True))
    v.update(("grad:" + k, _np(g)) for k, g in m.named_grads().items())
    sd = m.state_dict()
    v.update((k, _np(sd[k])) for k in danet_stat_names(sd))
    return v, m, xd, td


def _newrale_model(variant, L, B, p32, pa32, device):
    from ecg_denoise_amd import NewRALE, RALENet
    inner = RALENet(variant, leads=2, L=L, max_batch=B, train=True, device=device)
    inner.load_state_dict(p32, strict=False)
    m = NewRALE(inner)
    m.load_state_dict(pa32)
    return m.train()


def run_newrale(case, seed, device):
    """One train step of the 12-lead adapter around a frozen RA-LENet -> (vals, the model in eval mode): y in train mode, loss /
    SNR / RMSE over the 12 x L windows, the eight adapter gradients, the inner BatchNorm's running statistics after the step
    (quirk A16: the frozen model's BatchNorm keeps training) and the eval-mode forward on those statistics."""
    variant, L, B = case
    p32, pa32, x, tgt = make_newrale_case(variant, L, B, seed)
    m = _newrale_model(variant, L, B, p32, pa32, device)
    xd, td = x.to(device), tgt.to(device)
    y = m(xd)
    loss, snr, rmse = m.loss_and_metrics(y, td)
    m.backward()
    torch.cuda.synchronize()
    v = OrderedDict(y=_np(y), loss=_np(loss), snr=_np(snr), rmse=_np(rmse))
    v.update(("grad:" + k, _np(g)) for k, g in zip(pa32, m.named_grads().values()))
    st = m.rale.state_dict()
    v["bn_mean"], v["bn_var"] = _np(st["conv1.2.running_mean"]), _np(st["conv1.2.running_var"])
    m.eval()
    v["y_eval"] = _np(m(xd))
    return v, m


def run_newrale_parity(variant, L, B, device="cuda:0", input_seed=2023):
    """-> dict of errors (parity_bars.errors) of run_newrale against step("newrale", ...), the fp64 oracle"""
    case = (variant, L, B)
    return errors(run_newrale(case, input_seed, device)[0], step("newrale", case, torch.float64, input_seed).vals)


def run_newrale_adam(variant, L, B, steps=3, device="cuda:0"):
    """`steps` train_steps of a fresh adapter against as many O.train_step / O.adam_step iterations on the adapter parameters
    in fp64 -> (dict of relative errors: "loss<i>", "pred<i>" per step, "param:<name>" after the last one; the model; the inner
    model's flat parameters before the first step)."""
    p32, pa32, x, tgt = make_newrale_case(variant, L, B)
    m = _newrale_model(variant, L, B, p32, pa32, device)
    xd, td = x.to(device), tgt.to(device)
    inner_before = m.rale.eng.params.clone()
    p = OrderedDict((k, v.double()) for k, v in p32.items())
    pa = OrderedDict((k, v.double()) for k, v in pa32.items())
    am = OrderedDict((k, torch.zeros_like(v)) for k, v in pa.items())
    av = OrderedDict((k, torch.zeros_like(v)) for k, v in pa.items())
    bn = O.new_bn_state(8, torch.float64)
    res = OrderedDict()
    for i in range(1, steps + 1):
        out = m.train_step(xd, td)
        ref = O.train_step(pa, x.double(), tgt.double(), lambda leaves, xx: O.newrale_forward(leaves, p, xx, variant, True, bn), am, av, i)
        res[f"loss{i}"] = abs(out["loss"].item() - ref["loss"].item()) / abs(ref["loss"].item())
        res[f"pred{i}"] = rel(out["pred"].cpu().numpy(), ref["pred"].numpy())
    torch.cuda.synchronize()
    for k, v in m.named_parameters():
        res["param:" + k] = rel(v.cpu().numpy(), pa[k].numpy())
    return res, m, inner_before


def oracle_windows(p32, x, tgt, idx, variant="full"):
    """fp64 oracle of a whole-batch train step whose output gradient is zero outside the windows `idx` (dy[idx] = d mse / d y
    of the whole batch): the BatchNorm statistics come from the WHOLE batch (the stem conv of every window is cheap on the CPU),
    the transformer stack runs on the picked windows only, and the BatchNorm backward - the one place where the other
    windows see the gradient - is reproduced by hand.  -> (pred of the windows `idx`, {parameter name: gradient})."""
    import torch.nn.functional as F
    from test_dp_gloo import _rest_of_network
    B, L = x.shape[0], x.shape[2]
    n = x.shape[1] * L
    sl = idx if isinstance(idx, slice) else torch.as_tensor(list(idx), dtype=torch.long)
    p = OrderedDict((k, v.double().requires_grad_(True)) for k, v in p32.items())
    a0 = F.leaky_relu(F.conv1d(x.double(), p["conv1.0.weight"], p["conv1.0.bias"], padding=1), 0.2)   # (B, 8, L)
    cnt = B * L
    mean = a0.detach().sum((0, 2)) / cnt
    var = (a0.detach() ** 2).sum((0, 2)) / cnt - mean ** 2
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    xhat = (a0.detach() - mean[None, :, None]) * rstd[None, :, None]
    x0 = (xhat[sl] * p["conv1.2.weight"].detach()[None, :, None] + p["conv1.2.bias"].detach()[None, :, None]).requires_grad_(True)
    pred = _rest_of_network(p, x0, variant)
    loss = ((pred - tgt[sl].double()) ** 2).sum() / (B * n)
    names = [k for k in p if not k.startswith("conv1.")]
    gs = torch.autograd.grad(loss, [x0] + [p[k] for k in names], allow_unused=True)
    gx0 = torch.zeros_like(a0.detach()); gx0[sl] = gs[0]
    s1, s2 = gx0.sum((0, 2)) / cnt, (gx0 * xhat).sum((0, 2)) / cnt
    da = p["conv1.2.weight"].detach()[None, :, None] * rstd[None, :, None] * (gx0 - s1[None, :, None] - xhat * s2[None, :, None])
    gw, gb = torch.autograd.grad(a0, [p["conv1.0.weight"], p["conv1.0.bias"]], da)
    want = {k: (g if g is not None else torch.zeros_like(p[k])) for k, g in zip(names, gs[1:])}
    want["conv1.0.weight"], want["conv1.0.bias"] = gw, gb
    want["conv1.2.weight"], want["conv1.2.bias"] = (gx0 * xhat).sum((0, 2)), gx0.sum((0, 2))
    return pred.detach(), want


def window_grad_errors(named_grads, want):
    """relative L2 error of every parameter gradient of the library against `want` (oracle_windows)"""
    err = OrderedDict()
    for k, g in want.items():
        mine = named_grads[k].cpu().numpy()
        if k.endswith("to_kv.bias"):
            C_ = mine.size // 2          # the key half is identically zero (softmax shift invariance): the value half
            e = rel(mine[C_:], g.numpy()[C_:])
        elif k == "conv1.0.bias":
            continue          # exactly zero through a BatchNorm: rounding noise on both sides
        else:
            e = rel(mine, g.numpy()) if g.norm().item() > 1e-14 else 0.0
        err[k] = e
    return err
