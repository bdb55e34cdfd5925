"""Shared helpers of the GPU parity tests: run the HIP path and the CPU oracle on the
same seeded inputs and report relative L2 errors per tensor."""
import functools
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import torch

import ralenet_oracle as O


def rel(a, b):
    a = np.asarray(a, dtype=np.float64).ravel(); b = np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def oracle_trace(p, x, variant, bn, dtype=torch.float64):
    """Oracle forward (training mode) that also returns every block / resample output,
    named like the library's debug tensors."""
    import math
    import torch.nn.functional as F
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


def compare_grads(ng, p, grads):
    """relative L2 error per parameter gradient: the library's `named_grads()` against the oracle's `grads` (in the order of `p`)"""
    gerr = OrderedDict()
    for (k, _), g in zip(p.items(), grads):
        g = torch.zeros_like(p[k]) if g is None else g
        gn = g.norm().item()
        mine = ng[k].cpu().numpy()
        if k.endswith("to_kv.bias"):
            # key-bias gradient is identically zero (softmax shift invariance): compare the value half,
            # and bound the key half by rounding noise
            C = mine.size // 2
            gerr["grad:" + k + "[v]"] = rel(mine[C:], g.numpy()[C:])
            gerr["gradabs:" + k + "[k]"] = float(np.abs(mine[:C]).max())
        else:
            gerr["grad:" + k] = rel(mine, g.numpy()) if gn > 1e-12 else float(np.abs(mine).max())
    return gerr


STEM_MARGIN = 1e-5          # the smallest |stem pre-activation| a parity case may have (about 100 roundings of an O(1) sum)


def stem_margin(variant, leads, L, B, seed=1234, params=None, input_seed=2023):
    """the smallest |stem pre-activation| of the case in fp64: its distance from the kink of the stem's LeakyReLU(0.2)"""
    import torch.nn.functional as F
    p32, x, _ = make_case(variant, leads, L, B, seed, input_seed=input_seed)
    if params is not None:
        p32 = params(p32)
    return F.conv1d(x.double(), p32["conv1.0.weight"].double(), p32["conv1.0.bias"].double(), padding=1).abs().min().item()


def oracle_step(variant, leads, L, B, seed=1234, params=None, dtype=torch.float64, gelu=None, input_seed=2023):
    return _oracle_step(variant, leads, L, B, seed, params, dtype, gelu, input_seed)


@functools.lru_cache(maxsize=8)
def _oracle_step(variant, leads, L, B, seed, params, dtype, gelu, input_seed):
    """One train step and the eval forward after it in the oracle alone, in `dtype`, on make_case's parameters (through `params`,
    a callable p32 -> p32, when given) and inputs.  `gelu` stands in for O.gelu during the call (the mutants of
    tests/test_parity_bars_cpu.py).  Cached and shared between run_parity and parity_yardstick: read-only for every caller.
    -> namespace: p (leaves), bn (state after the step), y, tr (oracle_trace's tensors), loss, snr, rmse, grads (in the order
    of p, None where unused), dx, y_eval."""
    p32, x, tgt = make_case(variant, leads, L, B, seed, input_seed=input_seed)
    if params is not None:
        p32 = params(p32)
    p = OrderedDict((k, v.to(dtype).requires_grad_(True)) for k, v in p32.items())
    bn = O.new_bn_state(8, dtype)
    xo = x.to(dtype).requires_grad_(True)
    t = tgt.to(dtype)
    keep = O.gelu
    if gelu is not None:
        O.gelu = gelu
    try:
        yo, tr = oracle_trace(p, xo, variant, bn)
        lo = O.mse(yo, t)
        *grads, dxo = torch.autograd.grad(lo, list(p.values()) + [xo], allow_unused=True)
        p = OrderedDict((k, v.detach()) for k, v in p.items())
        with torch.no_grad():
            y_eval = O.ralenet_forward(p, x.to(dtype), variant, training=False, bn=bn)
    finally:
        O.gelu = keep
    yo = yo.detach()
    return SimpleNamespace(p=p, bn=bn, y=yo, tr=OrderedDict((k, v.detach()) for k, v in tr.items()), loss=lo.detach(),
                           snr=O.snr(t, yo), rmse=O.rmse(t, yo), grads=grads, dx=dxo, y_eval=y_eval)


def oracle_parity(variant, leads, L, B, seed=1234, params=None, eval_forward=False, trace=True, gelu=None, input_seed=2023):
    """run_parity with the fp32 oracle (torch on the CPU, fp32 leaves and BatchNorm state) in the place of the HIP path: the same
    keys, each the relative error of the fp32 evaluation against the fp64 one.  `grad:input_frozen` and the `@dx` stem gradients
    repeat `grad:input` and the stem gradients (the oracle has one backward pass).  `gelu` replaces O.gelu in the fp32
    evaluation only."""
    a = oracle_step(variant, leads, L, B, seed, params, torch.float32, gelu, input_seed)
    o = oracle_step(variant, leads, L, B, seed, params, torch.float64, None, input_seed)
    res = OrderedDict()
    res["y"] = rel(a.y.numpy(), o.y.numpy())
    res["loss"] = abs(a.loss.item() - o.loss.item()) / abs(o.loss.item())
    res["snr"] = rel(a.snr.numpy(), o.snr.numpy())
    res["rmse"] = rel(a.rmse.numpy(), o.rmse.numpy())
    res["bn_mean"] = rel(a.bn["running_mean"].numpy(), o.bn["running_mean"].numpy())
    res["bn_var"] = rel(a.bn["running_var"].numpy(), o.bn["running_var"].numpy())
    if trace:
        for k, v in o.tr.items():
            res["act:" + k] = rel(a.tr[k].numpy(), v.numpy())
    ng = OrderedDict((k, torch.zeros_like(a.p[k]) if g is None else g) for k, g in zip(a.p, a.grads))
    res.update(compare_grads(ng, o.p, o.grads))
    res["grad:input"] = rel(a.dx.numpy(), o.dx.numpy())
    stem = [k for k in o.p if k.startswith(("conv1.0.", "conv1.2."))]
    res.update(("grad:" + k + "@dx", res["grad:" + k]) for k in stem)
    res["grad:input_frozen"] = res["grad:input"]
    if eval_forward:
        res["y_eval"] = rel(a.y_eval.numpy(), o.y_eval.numpy())
    return res


THREE_SEEDS = (2023, 2024, 2025)


def parity_yardstick(variant, leads, L, B, seed=1234, params=None, eval_forward=False, trace=True, input_seeds=THREE_SEEDS):
    """What fp32 arithmetic itself costs, per tensor: a dict with the keys of run_parity(variant, leads, L, B, ...)'s result,
    each value rel(fp32 oracle, fp64 oracle) of that tensor on the same seeded parameters and inputs (oracle_parity).  It is
    the oracle's error, never the kernels'.  `gradabs:*` keys and gradients whose fp64 norm is <= 1e-12 get None: a quantity whose
    true value is zero has no relative yardstick, and keeps its flat absolute bar.

    One fp32 evaluation is a single sample of each tensor's rounding error, and torch's summation order follows the thread
    count: the three-element `leconv.partial_conv3.weight` gradients came out between 1.1e-7 and 5.5e-7 for the same case at 16
    threads and at 1, the nearly cancelling attention query gradients of the spread cases vary fivefold from one input to the
    next - and the strict f16_split = 0 path, whose summation order is its own, sat 8.5 to 8.6 times above such a sample.  So the
    yardstick is the largest of three fp32 evaluations, each against its own fp64 one, on inputs from the seeds `input_seeds`:
    2023 (the case's own), 2024 and 2025; the parameters stay.  parity_bars floors it at its group's median besides.

    Precondition: the stem's LeakyReLU(0.2) is the one kink of RA-LENet, and an fp32 pre-activation on the other side of 0
    from the fp64 one changes gradients by a discrete amount no yardstick describes - the smallest |stem pre-activation| of the
    case (fp64) must be >= STEM_MARGIN."""
    assert input_seeds[0] == 2023
    margin = stem_margin(variant, leads, L, B, seed, params)
    assert margin >= STEM_MARGIN, (variant, leads, L, B, margin)
    o = oracle_step(variant, leads, L, B, seed, params, torch.float64)
    yard = oracle_parity(variant, leads, L, B, seed, params, eval_forward, trace)
    for s in input_seeds[1:]:
        # (the other inputs are no parity case and owe no margin: it is enough that no fp32 pre-activation changed sides)
        a0, a1 = (oracle_step(variant, leads, L, B, seed, params, dt, None, s).tr["a0"] for dt in (torch.float32, torch.float64))
        assert torch.equal(a0 > 0, a1 > 0), (variant, leads, L, B, s)
        more = oracle_parity(variant, leads, L, B, seed, params, eval_forward, trace, None, s)
        yard = OrderedDict((k, max(v, more[k])) for k, v in yard.items())
    zero = {k for k, g in zip(o.p, o.grads) if g is None or g.norm().item() <= 1e-12}
    for k in yard:
        if k.startswith("gradabs:") or (k.startswith("grad:") and k[5:].split("@")[0] in zero):
            yard[k] = None
    return yard


def _group(key):
    return 1 if key.startswith("grad:") else 0


def yardstick_floors(yard):
    """-> (median of the non-None yardsticks of the forward group, of the gradient group)"""
    return tuple(float(np.median([v for k, v in yard.items() if v is not None and _group(k) == g])) for g in (0, 1))


def parity_bars(yard, K=8.0, flat=(1e-5, 1e-4), capped=True):
    """One bar per key of `yard`: min(flat bar of the key's group, K * max(yard[key], median of yard over the group)); the
    groups are the gradients (`grad:*`, flat[1]) and everything else (flat[0]).  A key without a yardstick (None) has the flat bar.

    K = 8: the design lets an fp16-pair product be 2^-21 relative where fp32 rounds at 2^-24 (csrc/ral_device.hpp, DESIGN.md
    section 4), so a tensor may carry 2^3 times the error of an fp32 evaluation and no more.  The median floor: the smallest
    single samples (4.5e-8 .. 1e-7, at small tensors) say little about the tensor's typical rounding error.  The min keeps every
    bar at or below the flat one; `capped=False` drops it, for cases whose tensors are ill conditioned in fp32 itself (the
    yardstick of such a tensor is above the flat bar, and so is what any fp32 kernel can reach)."""
    floors = yardstick_floors(yard)
    bars = OrderedDict()
    for k, v in yard.items():
        g = _group(k)
        if v is None:
            bars[k] = flat[g]
        else:
            bars[k] = K * max(v, floors[g])
            if capped:
                bars[k] = min(flat[g], bars[k])
    return bars


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


def run_parity(variant, leads, L, B, device="cuda:0", trace=True, seed=1234, options=None, eval_forward=False, before_forward=None,
               params=None):
    """-> dict of relative errors (HIP fp32 vs fp64 oracle).  `options`: {name: value} for ral_set_option on the model's handle,
    applied before the first forward.  `params`: a callable p32 -> p32 applied to the seeded parameters before the model and the
    oracle see them (spread_fc1_bias).  `eval_forward`: after the train step, the eval-mode forward of the same model against
    the oracle's eval output (its BatchNorm on the running statistics the step left) as res["y_eval"].  `before_forward(model)`
    is called once the options are set.  Gradients: every parameter gradient of `backward()` (dx = NULL, the training default);
    then res["grad:input"] and the stem parameter gradients "grad:<name>@dx" of `backward(want_dx=True)`, and
    res["grad:input_frozen"] of `backward_input` - the model comes back with the gradient buffer that last call left."""
    from ecg_denoise_amd import RALENet, _lib
    p32, x, tgt = make_case(variant, leads, L, B, seed)
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
    # fp64 oracle (x is a leaf: the input gradient comes out of the same autograd call); shared with parity_yardstick
    o = oracle_step(variant, leads, L, B, seed, params, torch.float64)
    p, bn, yo, tr, lo, grads, dxo = o.p, o.bn, o.y, o.tr, o.loss, o.grads, o.dx
    res = OrderedDict()
    res["y"] = rel(y.cpu().numpy(), yo.detach().numpy())
    res["loss"] = abs(loss.item() - lo.item()) / abs(lo.item())
    res["snr"] = rel(snr.cpu().numpy(), O.snr(tgt.double(), yo.detach()).numpy())
    res["rmse"] = rel(rmse.cpu().numpy(), O.rmse(tgt.double(), yo.detach()).numpy())
    st = model.state_dict()
    res["bn_mean"] = rel(st["conv1.2.running_mean"].cpu().numpy(), bn["running_mean"].numpy())
    res["bn_var"] = rel(st["conv1.2.running_var"].cpu().numpy(), bn["running_var"].numpy())
    if trace:
        for k, v in tr.items():
            res["act:" + k] = rel(model.debug_tensor(k).cpu().numpy()[:v.numel()], v.detach().numpy())
    res.update(compare_grads(model.named_grads(), p, grads))
    # the backward pass again on the same saved forward, now with the input gradient (ral_backward zeroes the gradient buffer
    # itself): the stem kernel that formed only parameter gradients above stores dz as well - its parameter gradients are compared
    # again, as grad:<name>@dx - and k_conv1_bwd_dx turns dz into dx
    dx = model.backward(want_dx=True)
    torch.cuda.synchronize()
    res["grad:input"] = rel(dx.cpu().numpy(), dxo.numpy())
    stem = [k for k in p if k.startswith(("conv1.0.", "conv1.2."))]
    again = compare_grads(model.named_grads(), OrderedDict((k, p[k]) for k in stem), [grads[list(p).index(k)] for k in stem])
    res.update((k + "@dx", v) for k, v in again.items())
    # the frozen-weight chain (what NewRALE training runs: no weight-gradient kernels) from the same dy
    dxf = model.backward_input(model._dy)
    torch.cuda.synchronize()
    res["grad:input_frozen"] = rel(dxf.cpu().numpy(), dxo.numpy())
    if eval_forward:
        model.eval()
        ye = model(xd)
        torch.cuda.synchronize()
        res["y_eval"] = rel(ye.cpu().numpy(), o.y_eval.numpy())
        model.train()
    return res, model, (p32, x, tgt)


def make_newrale_case(variant, L, B, input_seed=2023):
    """`make_case`'s seeds for the 12-lead adapter: inner 2-lead RA-LENet parameters (1234), adapter parameters (77), x and
    target (B, 12, L) from generator `input_seed`"""
    p32 = O.init_params(O.ralenet_param_shapes(variant, 2), 1234)
    pa32 = O.init_params(O.newrale_param_shapes(), 77)
    g = torch.Generator().manual_seed(input_seed)
    x = torch.randn(B, 12, L, generator=g)
    tgt = torch.randn(B, 12, L, generator=g)
    return p32, pa32, x, tgt


def _newrale_model(variant, L, B, p32, pa32, device):
    from ecg_denoise_amd import NewRALE, RALENet
    inner = RALENet(variant, leads=2, L=L, max_batch=B, train=True, device=device)
    inner.load_state_dict(p32, strict=False)
    m = NewRALE(inner)
    m.load_state_dict(pa32)
    return m.train()


def run_newrale_parity(variant, L, B, device="cuda:0", input_seed=2023):
    """One train step of the 12-lead adapter around a frozen RA-LENet (HIP fp32) against the fp64 oracle -> dict of relative
    errors: y in train mode, loss / SNR / RMSE over the 12 x L windows, the eight adapter gradients ("grad:<name>"), the inner
    BatchNorm's running statistics after the step (quirk A16: the frozen model's BatchNorm keeps training) and the eval-mode
    forward on those statistics."""
    p32, pa32, x, tgt = make_newrale_case(variant, L, B, input_seed)
    m = _newrale_model(variant, L, B, p32, pa32, device)
    xd, td = x.to(device), tgt.to(device)
    y = m(xd)
    loss, snr, rmse = m.loss_and_metrics(y, td)
    m.backward()
    torch.cuda.synchronize()
    p = OrderedDict((k, v.double()) for k, v in p32.items())
    pa = OrderedDict((k, v.double().requires_grad_(True)) for k, v in pa32.items())
    bn = O.new_bn_state(8, torch.float64)
    yo = O.newrale_forward(pa, p, x.double(), variant, True, bn)
    lo = O.mse(yo, tgt.double())
    grads = torch.autograd.grad(lo, list(pa.values()))
    res = OrderedDict()
    res["y"] = rel(y.cpu().numpy(), yo.detach().numpy())
    res["loss"] = abs(loss.item() - lo.item()) / abs(lo.item())
    res["snr"] = rel(snr.cpu().numpy(), O.snr(tgt.double(), yo.detach()).numpy())
    res["rmse"] = rel(rmse.cpu().numpy(), O.rmse(tgt.double(), yo.detach()).numpy())
    for (k, g), mine in zip(zip(pa, grads), m.named_grads().values()):
        res["grad:" + k] = rel(mine.cpu().numpy(), g.numpy())
    st = m.rale.state_dict()
    res["bn_mean"] = rel(st["conv1.2.running_mean"].cpu().numpy(), bn["running_mean"].numpy())
    res["bn_var"] = rel(st["conv1.2.running_var"].cpu().numpy(), bn["running_var"].numpy())
    m.eval()
    ye = m(xd)
    torch.cuda.synchronize()
    with torch.no_grad():
        yeo = O.newrale_forward(OrderedDict((k, v.detach()) for k, v in pa.items()), p, x.double(), variant, training=False, bn=bn)
    res["y_eval"] = rel(ye.cpu().numpy(), yeo.numpy())
    return res


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
