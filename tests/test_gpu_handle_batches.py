"""Handles of the four networks and of the 12-lead adapter at changing, ragged and loop-wrapping batch sizes, and in the
call orders a training loop can produce.

Every handle is sized by `max_batch`, keeps host state between calls (the U-Net's replica flags and scratch rows, DANet's
pass cache, the adapter's saved tensors) and every kernel loops over windows under a grid cap.  Three groups:

  a  one handle per network, a train step per entry of NETS[...]["batches"]; after every step y, loss, dx, every parameter
     gradient and the running statistics are those of a FRESH handle of exactly that batch (same parameters, same BatchNorm
     state), and the fresh handle is compared with the fp64 oracle.
  b  every pass of every window loop, free of activation kinks: eval y of the largest batch at windows of the first, a middle
     and the ragged last pass of each cap equals, bit for bit, eval y of those windows alone on a small handle; for ACDAE (no
     BatchNorm) y, dx and the parameter gradients of the batch against those of its parts as well.  One loop is not here: the
     fused U-Net inference kernel's (k_unet_infer, L = 256 .. 1024).  Its grid is a device question, so a batch that wraps it
     follows from the CU count: tests/test_gpu_unet_infer.py, at every shape of the kernel.
  c  call orders: each one either gives the numbers of the canonical order on a fresh handle, or is refused with a pinned
     text and leaves the handle usable.  Never other numbers without an error.

Bars.  Two handles (or one handle twice) against each other: bit for bit where the quantity is formed without float atomics
(ACDAE y and dx, eval y of DANet and the U-Net), else per tensor |a - b| <= 2e-5 |b| + 1e-9, the noise bar of
tests/test_gpu_schedule.py.  A gradient that is exactly zero in exact arithmetic (a bias in front of a batch-statistics
BatchNorm) is rounding noise on both sides, so a bar relative to it says nothing: it keeps the absolute bound of the
network's own oracle test (U-Net 2e-5, DANet 1e-5).  Fresh handle against the fp64 oracle: forward, loss and running
statistics 1e-5, gradients 1e-4 (relative L2), as tests/test_gpu_{acdae,danet,unet,newrale_parity}.py.  Above 512 windows the
gradient bar is max(1e-4, 4 x e32), the rule of test_unet_bench_batch_matches_fp64_oracle: e32 is what the oracle itself,
evaluated in fp32 on the CPU, deviates from its fp64 evaluation by (slope flips at activation kinks); the seeds below were
chosen on the CPU so that e32 <= 2.5e-4 at every such batch, which the test asserts - no bar exceeds 1e-3.  DANet at fewer
than 8 windows keeps the 2e-3 of tests/test_gpu_danet.py (a BatchNorm over 2 descriptors divides by the variance of two
samples).

Window lengths are the shortest each network takes, so that batches past the caps stay small.

Observed on an MI355X (fresh handle against the fp64 oracle; e32 / gradient bar / worst gradient error; forward, loss and
running statistics never above 1.6e-6):
  ACDAE    1030: 5.1e-5 / 2.0e-4 / 1.05e-4 (dx)   513: 9.9e-5 / 4.0e-4 / 1.48e-4 (dx)   1024, 1025: 5.1e-5 / 2.0e-4 / 1.05e-4
           3: 3.2e-7   1: 1.6e-6 (bar 1e-4)
  DANet    4100: 6.4e-5 / 2.5e-4 / 1.9e-5   4097: 6.7e-5 / 2.7e-4 / 2.1e-5   1025: 2.7e-5 / 1.1e-4 / 7.4e-6
           513: 5.3e-5 / 2.1e-4 / 1.2e-5   37: 2.5e-6 (bar 1e-4)   2: 3.6e-4 (bar 2e-3; e32 there 3.1e-4)
  U-Net    (2, 64) 1030: 2.9e-5 / 1.2e-4 / 3.1e-5   1025: 1.7e-5 / 1.0e-4 / 4.2e-5   1: 3.0e-5   2, 5: 4.3e-6
           2050: 7.6e-5 / 3.0e-4 / 4.4e-5   (2, 48): 7.1e-5 at 1 window, else 4.2e-6   (2, 320): 1.3e-6
  adapter  8, 3, 1 windows: 5.4e-6
Shared handle against fresh handle, and fresh handle twice, as a fraction of the noise bar (worst over several runs of the
suite): ACDAE 0.11, U-Net 0.18, adapter 0.005, DANet 0.41.  DANet reached 1.02 to 1.22 at 4100 windows while k_dn_act added its
per-channel BatchNorm sums in LDS as floats: the order of those atomics varies, mean and rstd carried ~1e-7 of it, every
window's term moved with them, and the gradient of dec.DecoderList.3.activate.fcn.4.bias (two entries, norm 1.3e-4, a sum
over the batch that cancels to 1/3000 of its terms) showed it.  The accumulators are doubles now."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import danet_oracle as D
import ralenet_oracle as O
from parity_bars import FWD_TOL, GRAD_TOL
from parity_util import DANET_ZERO, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E32_MAX = 2.5e-4
ZERO_GRAD_ABS = {"unet": 2e-5, "danet": 1e-5}
REFUSAL = {"ralenet": "RA-LENet backward must follow a training forward: the last forward was an eval one",
           "unet": "U-Net backward must follow a training forward: the last forward was an eval one",
           "danet": "DANet backward needs a training forward of the same batch first"}

# kind, leads, L, max_batch, batches of (a), parameter seed, data seed.  The adapter wraps RA-LENet "full", whose R-wave tables need
# L >= 32: that is its shortest legal length
NETS = OrderedDict([
    ("acdae", dict(kind="acdae", leads=2, L=64, max_batch=1030, batches=(1030, 3, 1, 513, 1024, 1025, 1030), seed=1234, data=2023)),
    ("danet", dict(kind="danet", leads=2, L=32, max_batch=4100, batches=(4100, 2, 37, 513, 1025, 4097, 4100), seed=7, data=1079)),
    ("unet_fold", dict(kind="unet", leads=2, L=64, max_batch=1030, batches=(1030, 1, 5, 1025, 2, 1030), seed=1234, data=2023)),
    ("unet_atomic", dict(kind="unet", leads=2, L=48, max_batch=6, batches=(6, 1, 5, 6), seed=1234, data=2023)),
    ("unet_staged", dict(kind="unet", leads=2, L=320, max_batch=4, batches=(4, 1, 4), seed=1234, data=2023)),
    ("newrale", dict(kind="newrale", leads=12, L=32, max_batch=8, batches=(8, 1, 3, 8), seed=1234, data=2023)),
])
# (b): windows of the first, a middle and the ragged last pass of every cap the network's kernels loop under
PASS_WINDOWS = {
    "acdae": (0, 1, 300, 511, 512, 513, 1023, 1024, 1025, 1029),                     # caps 512 and 1024
    "danet": (0, 5, 511, 512, 1023, 1024, 1025, 2047, 2048, 3071, 3072, 4095, 4096, 4097, 4099),   # 512, 1024, 256 x 4, 256 x 16
    "unet_fold": (0, 1, 2, 3, 343, 344, 511, 512, 1023, 1024, 1026, 1027, 1028, 1029),   # 344 workgroups x 3 windows; 512 x 2
    "unet_atomic": (0, 3, 5),
    "unet_staged": (0, 2, 3),
    "newrale": (0, 3, 7),
    "unet_wrap": (0, 1, 2047, 2048, 2049),
    "unet_fused": (0, 1, 3),      # one window per workgroup; the wrapped loop of k_unet_infer: tests/test_gpu_unet_infer.py
}
# beyond the lists of (a): the U-Net's forward stage kernels take up to 4 windows per pass on 512 workgroups, so their loop wraps
# beyond 2048 windows only, and k_unet_out_loss gives a wave a second window per pass only there (tests/test_handle_batches_cpu.py)
UNET_WRAP = dict(kind="unet", leads=2, L=64, max_batch=2050, batches=(2050,), seed=1234, data=2023)
UNET_FUSED = dict(kind="unet", leads=2, L=256, max_batch=4, batches=(4,), seed=1234, data=2023)      # eval forward: one kernel
CFG = OrderedDict(NETS, unet_wrap=UNET_WRAP, unet_fused=UNET_FUSED)


# ---------------------------------------------------------------------------------------------------------------------
# data, models and oracles per network (everything here runs on the CPU except _model)
# ---------------------------------------------------------------------------------------------------------------------
def initial_state(name):
    """the state_dict every handle of `name` starts from (fp32, CPU)"""
    n = CFG[name]
    if n["kind"] == "acdae":
        return O.init_params(O.acdae_param_shapes(), n["seed"])
    if n["kind"] == "unet":
        return O.init_params(O.unet_param_shapes(n["leads"]), n["seed"])
    if n["kind"] == "danet":
        return D.init_state(n["seed"], leads=n["leads"])
    sd = OrderedDict(O.init_params(O.newrale_param_shapes(), 77))
    sd.update(("rale." + k, v) for k, v in O.init_params(O.ralenet_param_shapes("full", 2), n["seed"]).items())
    return sd


_DATA = {}


def data(name, B, other=False):
    """the first B windows of the network's pool (x, target), CPU fp32; `other`: the pool in reverse order"""
    n = CFG[name]
    if name not in _DATA:
        g = torch.Generator().manual_seed(n["data"])
        _DATA[name] = (torch.randn(n["max_batch"], n["leads"], n["L"], generator=g), torch.randn(n["max_batch"], n["leads"], n["L"], generator=g))
    x, t = _DATA[name]
    if other:
        x, t = x.flip(0), t.flip(0)
    return x[:B].contiguous(), t[:B].contiguous()


def is_running(k):
    return k.endswith("running_mean") or k.endswith("running_var")


def oracle_step(name, sd, x, t, dtype=torch.float64, training=True):
    """one training forward + loss + backward of the oracle from the state_dict `sd` -> dict(y, loss, grads {name: tensor},
    dx (None where the network forms none), state {key: running statistic after the step}); training = False: y only"""
    kind = CFG[name]["kind"]
    cast = lambda v: v.detach().clone().to(dtype) if v.dtype.is_floating_point else v.clone()
    xd = x.detach().clone().to(dtype).requires_grad_(training and kind in ("acdae", "danet"))
    state = OrderedDict()
    if kind == "acdae":
        p = OrderedDict((k, cast(sd[k]).requires_grad_(training)) for k in O.acdae_param_shapes())
        y = O.acdae_forward(p, xd)
    elif kind == "unet":
        p = OrderedDict((k, cast(sd[k]).requires_grad_(training)) for k in O.unet_param_shapes(CFG[name]["leads"]))
        bn = O.unet_bn_state(p, dtype)
        for k in O.UNET_BN:
            for s in ("running_mean", "running_var"):
                if k + "." + s in sd:
                    bn[k][s] = cast(sd[k + "." + s])
        y = O.unet_forward(p, xd, training, bn)
        state = OrderedDict((k + "." + s, bn[k][s]) for k in O.UNET_BN for s in ("running_mean", "running_var"))
    elif kind == "danet":
        st = OrderedDict((k, cast(v)) for k, v in sd.items() if ".dam.fcn2." not in k)
        p = OrderedDict((k, v.requires_grad_(training)) for k, v in st.items() if D.is_param(k))
        y = D.danet_forward(st, xd, training=training)
        state = OrderedDict((k, v) for k, v in st.items() if is_running(k))
    else:
        p = OrderedDict((k, cast(sd[k]).requires_grad_(training)) for k in O.newrale_param_shapes())
        inner = OrderedDict((k, cast(sd["rale." + k])) for k in O.ralenet_param_shapes("full", 2))
        bn = O.new_bn_state(8, dtype)
        for s in ("running_mean", "running_var"):
            if "rale.conv1.2." + s in sd:
                bn[s] = cast(sd["rale.conv1.2." + s])
        y = O.newrale_forward(p, inner, xd, "full", training, bn)
        state = OrderedDict(("rale.conv1.2." + s, bn[s]) for s in ("running_mean", "running_var"))
    if not training:
        return {"y": y.detach()}
    loss = O.mse(y, t.to(dtype))
    gs = torch.autograd.grad(loss, list(p.values()) + ([xd] if xd.requires_grad else []), allow_unused=True)
    grads = OrderedDict((k, torch.zeros_like(v) if g is None else g) for (k, v), g in zip(p.items(), gs))
    return {"y": y.detach(), "loss": loss.item(), "grads": grads, "dx": gs[-1] if xd.requires_grad else None, "state": state}


_E32 = {}


def e32_of(name, B, ref=None):
    """what fp32 arithmetic itself costs at this batch: the oracle in fp32 on the CPU against its fp64 evaluation, the worst
    relative L2 deviation over the parameter gradients (those that are not identically zero) and the input gradient"""
    if (name, B) not in _E32:
        sd = initial_state(name)
        x, t = data(name, B)
        ref = ref or oracle_step(name, sd, x, t)
        o32 = oracle_step(name, sd, x, t, torch.float32)
        e = [rel(o32["grads"][k].numpy(), g.numpy()) for k, g in ref["grads"].items() if g.norm().item() >= 1e-9]
        if ref["dx"] is not None:
            e.append(rel(o32["dx"].numpy(), ref["dx"].numpy()))
        _E32[(name, B)] = max(e)
    return _E32[(name, B)]


def grad_bar(name, B, ref=None):
    """(gradient bar against the fp64 oracle, e32 or None)"""
    base = 2e-3 if CFG[name]["kind"] == "danet" and B < 8 else GRAD_TOL
    if B <= 512:
        return base, None
    e32 = e32_of(name, B, ref)
    return max(base, 4.0 * e32), e32          # (the caller asserts e32 <= E32_MAX, after it has printed its figures)


def _model(name, max_batch, sd):
    from ecg_denoise_amd import ACDAE, DANet, NewRALE, RALENet, UNet
    n = CFG[name]
    if n["kind"] == "acdae":
        m = ACDAE(L=n["L"], max_batch=max_batch, device=DEV)
    elif n["kind"] == "unet":
        m = UNet(leads=n["leads"], L=n["L"], max_batch=max_batch, device=DEV)
    elif n["kind"] == "danet":
        m = DANet(L=n["L"], max_batch=max_batch, device=DEV, leads=n["leads"])
    else:
        m = NewRALE(RALENet("full", leads=2, L=n["L"], max_batch=max_batch, device=DEV, seed=1), seed=2)
    m.load_state_dict(sd, strict=False)
    return m.train()


def _has_dx(name):
    return CFG[name]["kind"] in ("acdae", "danet")


def _grads(m):
    return OrderedDict((k, v.detach().clone()) for k, v in m.named_grads().items())


def _running(m):
    return OrderedDict((k, v.clone()) for k, v in m.state_dict().items() if is_running(k) and ".dam.fcn2." not in k)


def _backward(name, m, dy=None):
    if CFG[name]["kind"] == "newrale":
        m.backward(dy)
        return None
    return m.backward(dy, want_dx=_has_dx(name))


def _step(name, m, x, t, fused=False):
    """forward, loss, backward in training mode -> everything the step left, cloned.  `fused`: forward_loss + backward()"""
    m.train()
    if fused:
        y, loss, _, _ = m.forward_loss(x, t)
    else:
        y = m(x)
        loss, _, _ = m.loss_and_metrics(y, t)
    dx = _backward(name, m)
    torch.cuda.synchronize()
    return {"y": y.clone(), "loss": loss.item(), "dx": None if dx is None else dx.clone(), "grads": _grads(m), "state": _running(m)}


def _counters(m):
    return {k: int(v) for k, v in m.state_dict().items() if k.endswith("num_batches_tracked")}


def noise_ratio(a, b):
    """|a - b| / (2e-5 |b| + 1e-9) (pass: <= 1)"""
    a, b = torch.as_tensor(a).double().flatten().cpu(), torch.as_tensor(b).double().flatten().cpu()
    return (a - b).norm().item() / (2e-5 * b.norm().item() + 1e-9)


def _same_step(name, got, want, zero, what, exact_y=None, defer=None):
    """`got` against `want` (two handles, or one twice) under the bars of the module docstring -> the worst ratio to the noise
    bar.  `zero`: names of the gradients that are identically zero in exact arithmetic; `defer` as in _against_oracle"""
    kind = CFG[name]["kind"]
    exact = kind == "acdae" if exact_y is None else exact_y
    worst, bad = {}, {}
    for k in ("y", "dx"):
        if got[k] is None:
            continue
        if exact and not torch.equal(got[k], want[k]):
            bad[k + " bit for bit"] = noise_ratio(got[k], want[k])
        elif not exact:
            worst[k] = noise_ratio(got[k], want[k])
    worst["loss"] = abs(got["loss"] - want["loss"]) / (2e-5 * abs(want["loss"]) + 1e-9)
    for k, g in want["grads"].items():
        if k in zero:
            z = max(got["grads"][k].abs().max().item(), g.abs().max().item())
            if not z <= ZERO_GRAD_ABS[kind]:
                bad["zero gradient " + k] = z
        else:
            worst["grad:" + k] = noise_ratio(got["grads"][k], g)
    for k, v in want["state"].items():
        worst["state:" + k] = noise_ratio(got["state"][k], v)
    bad.update({k: v for k, v in worst.items() if not v <= 1.0})
    if defer is None:
        assert not bad, (what, bad)
    elif bad:
        defer.append((what, bad))
    return max(worst.values()) if worst else 0.0


def _against_oracle(name, B, got, ref, what, defer=None):
    """the fresh handle's step against the fp64 oracle -> (worst forward error, worst gradient error, bar, e32, zero-gradient names);
    `defer`: a list that takes what misses its bar, for a caller that goes through all its batches before it asserts"""
    kind = CFG[name]["kind"]
    bar, e32 = grad_bar(name, B, ref)
    fwd = {"y": rel(got["y"].cpu().numpy(), ref["y"].numpy()), "loss": abs(got["loss"] - ref["loss"]) / abs(ref["loss"])}
    for k, v in ref["state"].items():
        fwd["state:" + k] = rel(got["state"][k].cpu().numpy(), v.numpy())
    gerr, zerr, zero = {}, {}, set()
    for k, g in ref["grads"].items():
        mine = got["grads"][k].cpu().numpy()
        if g.norm().item() < 1e-9 or (kind == "danet" and k.endswith(DANET_ZERO)):
            zero.add(k)
            zerr[k] = float(np.abs(mine).max())
        else:
            gerr[k] = rel(mine, g.numpy())
    if ref["dx"] is not None:
        gerr["dx"] = rel(got["dx"].cpu().numpy(), ref["dx"].numpy())
    print(f"[handle] {what}: e32 {'-' if e32 is None else format(e32, '.2e')}, gradient bar {bar:.1e}, worst forward "
          f"{max(fwd.values()):.2e} ({max(fwd, key=fwd.get)}), worst gradient {max(gerr.values()):.2e} ({max(gerr, key=gerr.get)})")
    bad = {k: v for k, v in fwd.items() if not v < FWD_TOL}
    bad.update({k: v for k, v in gerr.items() if not v < bar})
    bad.update({"zero gradient " + k: v for k, v in zerr.items() if not v <= ZERO_GRAD_ABS[kind]})
    if e32 is not None and not e32 <= E32_MAX:
        bad["e32"] = e32
    if defer is None:
        assert not bad, (what, bad, bar)
    elif bad:
        defer.append((what, bad, bar))
    return max(fwd.values()), max(gerr.values()), bar, e32, zero


# ---------------------------------------------------------------------------------------------------------------------
# a: one handle, changing batches
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(NETS))
def test_changing_batches_on_one_handle(name):
    n = CFG[name]
    shared = _model(name, n["max_batch"], initial_state(name))
    forwards, missed = 0, []                                  # (every batch is measured and printed before anything is asserted)
    for i, B in enumerate(n["batches"]):
        what = f"{name} step {i} B={B}"
        x, t = data(name, B)
        xd, td = x.to(DEV), t.to(DEV)
        before = OrderedDict((k, v.cpu()) for k, v in shared.state_dict().items())
        fused = n["kind"] == "unet" and i % 2 == 1           # the U-Net alternates between its two ways through a step
        got = _step(name, shared, xd, td, fused)
        forwards += 1
        fresh = _model(name, B, before)
        want = _step(name, fresh, xd, td)
        ref = oracle_step(name, before, x, t)
        _, _, _, _, zero = _against_oracle(name, B, want, ref, what + " fresh handle", missed)
        fresh.load_state_dict(before, strict=False)
        again = _step(name, fresh, xd, td)
        noise = _same_step(name, again, want, zero, what + " fresh handle twice", defer=missed)
        worst = _same_step(name, got, want, zero, what + " shared handle", defer=missed)
        print(f"[handle] {what}{' (forward_loss)' if fused else ''}: shared against fresh {worst:.3f} of the noise bar, fresh twice {noise:.3f}")
        for k, c in _counters(shared).items():
            per = 2 if ".dam.fcn" in k else 1                # (DANet: the DAM's fcn sees two batches per forward)
            assert c == per * forwards, (what, k, c)
        if i % 2 == 1 and n["kind"] != "acdae":
            # eval y has no float atomics: bit for bit once both handles hold the same running statistics
            after = shared.state_dict()
            fresh.load_state_dict(after, strict=False)
            shared.eval(); fresh.eval()
            if not torch.equal(shared(xd), fresh(xd)):
                missed.append((what, "eval y differs between the shared and the fresh handle"))
            shared.train()
            assert _counters(shared) == {k: int(v) for k, v in after.items() if k.endswith("num_batches_tracked")}
        del fresh
    assert not missed, missed


# ---------------------------------------------------------------------------------------------------------------------
# b: every pass of every loop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CFG))
def test_eval_windows_of_every_pass_equal_the_windows_alone(name):
    n = CFG[name]
    B, idx = n["max_batch"], list(PASS_WINDOWS[name])
    assert idx[0] == 0 and idx[-1] == B - 1
    sd = initial_state(name)
    x, _ = data(name, B)
    big = _model(name, B, sd).eval()
    y = big(x.to(DEV)).clone()
    assert torch.isfinite(y).all()
    small = _model(name, len(idx), sd).eval()
    assert torch.equal(small(x[idx].contiguous().to(DEV)), y[idx]), name
    one = _model(name, 1, sd).eval()                            # ... and a window on its own
    for w in (idx[len(idx) // 2], idx[-1]):
        assert torch.equal(one(x[w:w + 1].contiguous().to(DEV)), y[w:w + 1]), (name, w)
    # against the oracle: the picked windows (eval mode: a window does not depend on its batch)
    yo = oracle_step(name, sd, x[idx], None, training=False)["y"]
    assert rel(y[idx].cpu().numpy(), yo.numpy()) < FWD_TOL


def test_unet_beyond_2048_windows_matches_oracle_in_both_call_forms():
    """2050 windows of 64 samples: the forward stage kernels run a second, ragged pass (512 workgroups x 4 windows, then 2), and
    in `forward_loss` two waves of k_unet_out_loss take a second window - both for the first time in the suite"""
    name, B = "unet_wrap", 2050
    sd = initial_state(name)
    x, t = data(name, B)
    xd, td = x.to(DEV), t.to(DEV)
    ref = oracle_step(name, sd, x, t)
    split = _step(name, _model(name, B, sd), xd, td)
    zero = _against_oracle(name, B, split, ref, "unet 2050 forward + loss + backward")[4]
    fused = _step(name, _model(name, B, sd), xd, td, fused=True)
    _against_oracle(name, B, fused, ref, "unet 2050 forward_loss + backward")
    _same_step(name, fused, split, zero, "unet 2050 forward_loss against forward + loss")


def test_acdae_batch_is_the_sum_of_its_ragged_parts():
    """no BatchNorm: in training mode too, y and dx of a slice are the slice's own on a handle of its size, bit for bit, and the
    parameter gradients of 1030 windows are the sums of those of 1024 + 6 and of 513 + 517 (the same upstream gradient)"""
    name, B = "acdae", 1030
    sd = initial_state(name)
    x, t = data(name, B)
    xd = x.to(DEV)
    dy = (t / t.numel()).to(DEV)
    m = _model(name, B, sd)
    y = m(xd).clone()
    dx = m.backward(dy, want_dx=True).clone()
    whole = _grads(m)
    for cuts in ((0, 1024, 1030), (0, 513, 1030)):
        total = None
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            h = _model(name, hi - lo, sd)
            assert torch.equal(h(xd[lo:hi].contiguous()), y[lo:hi]), (lo, hi)
            assert torch.equal(h.backward(dy[lo:hi].contiguous(), want_dx=True), dx[lo:hi]), (lo, hi)
            part = OrderedDict((k, v.double()) for k, v in _grads(h).items())
            total = part if total is None else OrderedDict((k, total[k] + part[k]) for k in part)
        r = {k: noise_ratio(whole[k], total[k]) for k in whole}
        print(f"[handle] acdae 1030 = {cuts[1]} + {cuts[2] - cuts[1]}: worst {max(r.values()):.3f} of the noise bar ({max(r, key=r.get)})")
        assert all(v <= 1.0 for v in r.values()), (cuts, {k: v for k, v in r.items() if v > 1.0})


# ---------------------------------------------------------------------------------------------------------------------
# c: call orders
# ---------------------------------------------------------------------------------------------------------------------
# batches of the call-order tests: a few windows, since these tests are about host state.  DANet takes 37, the smallest batch of
# its list above at which its bars hold with room: its BatchNorms over the batch of descriptors amplify fp32 rounding at a handful
# of windows (tests/test_gpu_danet.py: 2e-3 below 8), and with it the order-dependent noise of the float atomics of the weight
# gradients - at 9 and 19 windows two runs differed by up to 1.1 of the noise bar on the smallest bias gradients, at 37 by 0.26
ORDER_B = {"acdae": 5, "danet": 37, "unet_fold": 5, "unet_atomic": 5, "unet_staged": 3, "newrale": 3}


def _zero_names(name, ref):
    kind = CFG[name]["kind"]
    return {k for k, g in ref["grads"].items()
            if g.norm().item() < 1e-9 or (kind == "danet" and k.endswith(DANET_ZERO))}


def _canonical(name, B, sd, other=False):
    """the canonical order (forward, loss, backward) on a fresh handle of B windows -> (its step, the zero-gradient names)"""
    x, t = data(name, B, other)
    want = _step(name, _model(name, B, sd), x.to(DEV), t.to(DEV))
    return want, _zero_names(name, oracle_step(name, sd, x, t))


@pytest.mark.parametrize("name", list(NETS))
def test_two_training_forwards_then_backward(name):
    """training forward (B1), training forward (B2, other windows), loss, backward: the canonical step of B2 - nothing of the
    first forward's batch, records or saved tensors is left over.  B1 > B2 and B1 < B2."""
    cap = CFG[name]["max_batch"]
    small = ORDER_B[name]
    big = min(cap, 2 * small + 1)
    for B1, B2 in ((big, small), (small, big)):
        sd = initial_state(name)
        m = _model(name, cap, sd)
        m(data(name, B1)[0].to(DEV))
        before = OrderedDict((k, v.cpu()) for k, v in m.state_dict().items())      # (the first forward moved the running statistics)
        x, t = data(name, B2, other=True)
        got = _step(name, m, x.to(DEV), t.to(DEV))
        want, zero = _canonical(name, B2, before, other=True)
        _same_step(name, got, want, zero, f"{name} forward {B1}, forward {B2}, backward")


@pytest.mark.parametrize("name", ["acdae", "danet", "newrale"])
def test_backward_twice_gives_the_same_gradients(name):
    B = ORDER_B[name]
    sd = initial_state(name)
    x, t = data(name, B)
    m = _model(name, CFG[name]["max_batch"], sd)
    first = _step(name, m, x.to(DEV), t.to(DEV))
    dx = _backward(name, m)
    torch.cuda.synchronize()
    second = dict(first, dx=None if dx is None else dx.clone(), grads=_grads(m))
    want, zero = _canonical(name, B, sd)
    _same_step(name, first, want, zero, f"{name} first backward")
    _same_step(name, second, want, zero, f"{name} second backward")


def _refused_then_usable(name, m, B, fused=False):
    """training forward, loss, eval forward of the same B (the same windows, then others), backward: refused with the
    network's text; a canonical step afterwards is that of a fresh handle"""
    from ecg_denoise_amd import RalError
    kind = CFG[name]["kind"]
    text = REFUSAL["ralenet" if kind == "newrale" else kind]
    x, t = data(name, B)
    xd, td = x.to(DEV), t.to(DEV)
    for other in (False, True):
        m.train()
        if fused:
            m.forward_loss(xd, td)
        else:
            m.loss_and_metrics(m(xd), td)
        m.eval()
        m(data(name, B, other)[0].to(DEV))
        m.train()
        with pytest.raises(RalError, match=text):
            _backward(name, m)
        # the handle is still usable: the canonical step that follows is correct (the oracle bars of (a))
        before = OrderedDict((k, v.cpu()) for k, v in m.state_dict().items())
        got = _step(name, m, xd, td, fused)
        _against_oracle(name, B, got, oracle_step(name, before, x, t), f"{name} after the refusal (other={other}, fused={fused})")


@pytest.mark.parametrize("name", ["danet", "unet_fold", "unet_atomic", "unet_staged", "newrale"])
def test_backward_after_an_eval_forward_is_refused(name):
    """the eval forward keeps nothing a backward pass can use (RA-LENet: no lse; U-Net stage by stage: z[] overwritten with
    running-statistics activations; DANet: no batch sums): the backward is refused, whatever the eval forward's windows"""
    m = _model(name, CFG[name]["max_batch"], initial_state(name))
    _refused_then_usable(name, m, ORDER_B[name])
    if CFG[name]["kind"] == "unet":
        _refused_then_usable(name, m, ORDER_B[name], fused=True)


def test_unet_fused_eval_forward_refuses_the_backward_too():
    """L = 256: the eval forward is ONE kernel that touches neither z[] nor the records - the rule is the same as at every other
    length, so that one network does not behave in two ways depending on L"""
    name = "unet_fused"
    m = _model(name, CFG[name]["max_batch"], initial_state(name))
    _refused_then_usable(name, m, 3)
    _refused_then_usable(name, m, 3, fused=True)


def test_ralenet_backward_after_an_eval_forward_is_refused():
    """RA-LENet on its own handle (the adapter above reaches it through `backward_input` only): the eval forward writes no lse, so
    every way into the backward pass is refused after it, and the step that follows is that of a fresh handle"""
    from ecg_denoise_amd import RALENet, RalError
    import test_gpu_schedule as T
    p32 = O.init_params(O.ralenet_param_shapes("full", 2), 1234)
    g = torch.Generator().manual_seed(2023)
    x, t = torch.randn(3, 2, 32, generator=g).to(DEV), torch.randn(3, 2, 32, generator=g).to(DEV)
    m = RALENet("full", leads=2, L=32, max_batch=4, device=DEV); m.load_state_dict(p32, strict=False)
    for other in (False, True):
        m.train()
        m.loss_and_metrics(m(x), t)
        m.eval(); m(x.flip(0).contiguous() if other else x); m.train()
        for call in (m.backward, lambda: m.backward(want_dx=True), lambda: m.backward_input(m._dy)):
            with pytest.raises(RalError, match=REFUSAL["ralenet"]):
                call()
        before = m.state_dict()
        f = RALENet("full", leads=2, L=32, max_batch=3, device=DEV); f.load_state_dict(before)
        f.train()
        got, want = [], []
        for h, out in ((m, got), (f, want)):
            y = h(x); loss, _, _ = h.loss_and_metrics(y, t); dx = h.backward(want_dx=True)
            torch.cuda.synchronize()
            out += [y.clone(), loss.item(), dx.clone(), h.eng.grads.clone(), h.eng.state.clone()]
        assert torch.equal(got[0], want[0]) and got[1] == want[1] and torch.equal(got[4], want[4])
        assert noise_ratio(got[2], want[2]) <= 1.0
        T._assert_grads(m, got[3], want[3], f"after the refusal (other={other})")


def test_acdae_backward_after_an_eval_forward_is_that_forward_s():
    """ACDAE has no BatchNorm and keeps the same tensors in both modes: eval is the same function, so a backward after an eval
    forward is the backward of THAT forward (of its windows), bit for bit on dx"""
    name, B = "acdae", ORDER_B["acdae"]
    sd = initial_state(name)
    m = _model(name, CFG[name]["max_batch"], sd)
    x, t = data(name, B)
    for other in (False, True):
        x2, _ = data(name, B, other)
        m.train()
        y = m(x.to(DEV)); m.loss_and_metrics(y, t.to(DEV))
        dy = m._dy.clone()
        m.eval()
        y2 = m(x2.to(DEV)).clone()
        m.train()
        dx = m.backward(dy, want_dx=True).clone()
        got = _grads(m)
        f = _model(name, B, sd)
        assert torch.equal(f(x2.to(DEV)), y2)
        assert torch.equal(f.backward(dy, want_dx=True), dx)
        want = _grads(f)
        assert all(noise_ratio(got[k], want[k]) <= 1.0 for k in want), other


def _oracle_trainer(name, sd, dtype=torch.float64):
    """-> (parameters (updated in place by `step`), step(x, t, i) -> O.train_step's dict, running statistics)"""
    kind = CFG[name]["kind"]
    dd = lambda v: v.detach().clone().to(dtype)
    if kind == "acdae":
        p = OrderedDict((k, dd(sd[k])) for k in O.acdae_param_shapes())
        fwd, state = (lambda lv, xx: O.acdae_forward(lv, xx)), (lambda: {})
    elif kind == "unet":
        p = OrderedDict((k, dd(sd[k])) for k in O.unet_param_shapes(CFG[name]["leads"]))
        bn = O.unet_bn_state(p, dtype)
        fwd = lambda lv, xx: O.unet_forward(lv, xx, True, bn)
        state = lambda: {k + "." + s: bn[k][s] for k in O.UNET_BN for s in ("running_mean", "running_var")}
    elif kind == "danet":
        st = OrderedDict((k, dd(v) if v.dtype.is_floating_point else v.clone()) for k, v in sd.items() if ".dam.fcn2." not in k)
        p = OrderedDict((k, v) for k, v in st.items() if D.is_param(k))
        rest = OrderedDict((k, v) for k, v in st.items() if not D.is_param(k))
        fwd = lambda lv, xx: D.danet_forward(OrderedDict(list(rest.items()) + list(lv.items())), xx, training=True)
        state = lambda: {k: v for k, v in rest.items() if is_running(k)}
    else:
        p = OrderedDict((k, dd(sd[k])) for k in O.newrale_param_shapes())
        inner = OrderedDict((k, dd(sd["rale." + k])) for k in O.ralenet_param_shapes("full", 2))
        bn = O.new_bn_state(8, dtype)
        fwd = lambda lv, xx: O.newrale_forward(lv, inner, xx, "full", True, bn)
        state = lambda: {"rale.conv1.2." + s: bn[s] for s in ("running_mean", "running_var")}
    am = OrderedDict((k, torch.zeros_like(v)) for k, v in p.items())
    av = OrderedDict((k, torch.zeros_like(v)) for k, v in p.items())
    return p, (lambda x, t, i: O.train_step(p, x.to(dtype), t.to(dtype), fwd, am, av, i)), state


EPOCH_NETS = ["acdae", "danet", "unet_fold", "newrale"]
# data seeds of the epoch test, chosen on the CPU like the seeds of (a): DANet normalises over 3 descriptors in the ragged step, and
# on most seeds the oracle's own fp32 evaluation leaves the fp64 trajectory by more than the bars (seed 7: 4.4e-5 on the ninth
# prediction, seed 11: 9.5e-2).  With these the fp32 oracle stays within half of each bar, which the test asserts: the library's
# deviation and the fp32 oracle's are two roundings of the same trajectory, so one as accurate as the oracle keeps the bar.
EPOCH_SEED = {"acdae": 7, "danet": 24, "unet_fold": 7, "newrale": 7}
LOSS_RTOL, PRED_TOL, PARAM_TOL, STAT_TOL = 5e-4, 2e-5, 1e-5, 1e-5


def _mean_behind(bias):
    """the running mean of the BatchNorm right behind a conv / Linear bias"""
    if bias.endswith(".conv.bias"):
        return bias[:-len("conv.bias")] + "bn.running_mean"
    head, idx, _ = bias.rsplit(".", 2)
    return f"{head}.{int(idx) + 1}.running_mean"


@pytest.mark.parametrize("name", EPOCH_NETS)
def test_epochs_with_a_ragged_last_batch_and_eval_forwards_in_between(name):
    """three epochs as train() runs them on one handle of 8 windows: train steps of 8, 8 and 3 windows, then eval forwards of 8
    and 5 - against the oracle's Adam trajectory of the same nine steps WITHOUT the eval forwards.  Bars of
    tests/test_gpu_danet.py / test_gpu_newrale_parity.py: losses rtol 5e-4 (the golden tests'), prediction 2e-5, parameters
    1e-5, running statistics 1e-5.  Left out, as there: the biases in front of a batch-statistics BatchNorm (zero gradient: Adam
    turns their fp32 rounding noise into steps of up to lr) - and with them the running MEAN of that BatchNorm, which contains
    the bias as it stands (the running variance does not, and is compared).  The eval predictions after each epoch are compared
    at 2e-5 where the network has no such bias (ACDAE, the adapter); elsewhere eval mode subtracts a running mean that lags
    behind the wandering bias, so they are printed only."""
    n = CFG[name]
    sd = initial_state(name)
    m = _model(name, 8, sd)
    p, ostep, ostate = _oracle_trainer(name, sd)
    p32, ostep32, _ = _oracle_trainer(name, sd, torch.float32)
    g = torch.Generator().manual_seed(EPOCH_SEED[name])
    pool = [(torch.randn(B, n["leads"], n["L"], generator=g), torch.randn(B, n["leads"], n["L"], generator=g)) for B in (8, 8, 3)]
    ev = [torch.randn(B, n["leads"], n["L"], generator=g) for B in (8, 5)]
    zero, i = set(), 0
    loss, pred, own, evalp = [], [], [], []
    for epoch in range(3):
        m.train()
        for x, t in pool:
            i += 1
            out = m.train_step(x.to(DEV), t.to(DEV))
            ref, r32 = ostep(x, t, i), ostep32(x, t, i)
            zero |= {k for k, gr in ref["grads"].items() if gr.norm().item() < 1e-9}
            loss.append(abs(out["loss"].item() - ref["loss"].item()) / abs(ref["loss"].item()))
            pred.append(rel(out["pred"].cpu().numpy(), ref["pred"].numpy()))
            own.append(rel(r32["pred"].numpy(), ref["pred"].numpy()))
        m.eval()
        now = OrderedDict(sd)
        now.update((k, v.detach()) for k, v in p.items())
        now.update(ostate())
        for x in ev:
            evalp.append(rel(m(x.to(DEV)).cpu().numpy(), oracle_step(name, now, x, None, training=False)["y"].numpy()))
    torch.cuda.synchronize()
    if n["kind"] == "danet":
        zero |= {k for k in p if k.endswith(DANET_ZERO)}
    mine = dict(m.named_parameters())
    perr = {k: rel(mine[k].detach().cpu().numpy(), v.numpy()) for k, v in p.items() if k not in zero}
    pown = max(rel(p32[k].numpy(), v.numpy()) for k, v in p.items() if k not in zero)
    sdm = m.state_dict()
    skip = {_mean_behind(k) for k in zero}
    serr = {k: rel(sdm[k].cpu().numpy(), v.numpy()) for k, v in ostate().items() if k not in skip}
    assert len(skip) == len(zero) and all(k in sdm for k in skip)
    print(f"[handle] {name} 3 epochs: loss {max(loss):.2e}, prediction {max(pred):.2e} (step {1 + pred.index(max(pred))}), eval prediction "
          f"{max(evalp):.2e}, parameters {max(perr.values()):.2e}, running statistics {max(serr.values()) if serr else 0.0:.2e}; {len(zero)} "
          f"zero-gradient biases and the running means behind them left out; the oracle in fp32: prediction {max(own):.2e}, parameters {pown:.2e}")
    assert max(own) <= PRED_TOL / 2 and pown <= PARAM_TOL / 2, (max(own), pown)
    assert max(loss) <= LOSS_RTOL and max(pred) <= PRED_TOL and (zero or max(evalp) <= PRED_TOL), (loss, pred, evalp)
    assert all(v <= PARAM_TOL for v in perr.values()), {k: v for k, v in perr.items() if v > PARAM_TOL}
    assert all(v <= STAT_TOL for v in serr.values()), {k: v for k, v in serr.items() if v > STAT_TOL}
    for k, c in _counters(m).items():
        assert c == (18 if ".dam.fcn" in k else 9), (k, c)
