"""Fine-tuning with frozen BatchNorm statistics (library option "bn_frozen", `model.freeze_bn()`): a training-mode step that
normalises with the stored running statistics, leaves them alone and still trains every parameter - torch's `bn.eval()` with
autograd on.  The reference is the fp64 oracle with `training=False` under autograd.

Every model gets non-trivial statistics and affines first (running_mean in +-0.5, running_var in [0.5, 2], gamma in [0.5, 1.5],
beta in +-0.5, seeded): fresh 0 / 1 statistics would hide a swapped mean and variance, gamma = 1 a missing factor.

Bars: those of tests/test_gpu_parity.py (forward 1e-5, gradients 1e-4, relative L2 against fp64), for EVERY parameter - the
U-Net conv biases in front of a BatchNorm have real gradients here; the Adam loss trajectory at rtol 5e-4 (the bar of the
golden Adam trajectories); the split calls at 1e-4 against the one-call forms (test_split_ralenet / test_split_unet); the
autograd shim at the bars of tests/test_gpu_reference_loop.py (loss 2e-5, parameters 2e-4)."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import ralenet_oracle as O
from parity_bars import FWD_TOL, GRAD_TOL
from parity_util import compare_grads, make_case, make_newrale_case, rel
from test_unet_plan_cpu import query

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRAJ_RTOL = 5e-4                        # the golden Adam trajectories (test_gpu_parity.py, test_gpu_unet.py)
SPLIT_TOL = 1e-4                        # test_split_ralenet / test_split_unet
LOOP_LOSS_RTOL, LOOP_PARAM_TOL = 2e-5, 2e-4   # tests/test_gpu_reference_loop.py


def _lib():
    from ecg_denoise_amd import _lib as L
    return L


def with_statistics(p32, seed=99):
    """p32 + non-trivial BatchNorm affines and running statistics for every BatchNorm of the model (a 1-D `X.weight` whose
    shapes dictionary has no conv of that name is found by the oracle's lists) -> one dict for `load_state_dict`"""
    g = torch.Generator().manual_seed(seed)
    bns = ["conv1.2"] if "conv1.2.weight" in p32 else list(O.UNET_BN)
    sd = OrderedDict(p32)
    u = lambda n, lo, hi: lo + (hi - lo) * torch.rand(n, generator=g)
    for k in bns:
        n = p32[k + ".weight"].numel()
        sd[k + ".weight"] = u(n, 0.5, 1.5)
        sd[k + ".bias"] = u(n, -0.5, 0.5)
        sd[k + ".running_mean"] = u(n, -0.5, 0.5)
        sd[k + ".running_var"] = u(n, 0.5, 2.0)
    return sd, bns


def oracle_leaves(sd, bns):
    """-> (fp64 leaves of the parameters, the oracle's BatchNorm state holding the statistics of `sd`)"""
    p = OrderedDict((k, v.double().requires_grad_(True)) for k, v in sd.items() if "running_" not in k)
    state = {k: {"running_mean": sd[k + ".running_mean"].double(), "running_var": sd[k + ".running_var"].double(),
                 "num_batches_tracked": 0} for k in bns}
    return p, (state["conv1.2"] if bns == ["conv1.2"] else state)


def snapshot(model):
    """the running statistics (flat, a clone) and every num_batches_tracked"""
    torch.cuda.synchronize()
    return model.eng.state.clone(), dict(model.eng.counters)


def assert_untouched(model, snap):
    torch.cuda.synchronize()
    assert torch.equal(model.eng.state, snap[0]), "the running statistics were written"
    assert model.eng.counters == snap[1], "num_batches_tracked advanced"
    sd = model.state_dict()
    assert all(int(v) == 0 for k, v in sd.items() if k.endswith("num_batches_tracked"))


def check(res):
    bad = {}
    for k, v in res.items():
        tol = 1e-5 if k.startswith("gradabs:") else (GRAD_TOL if k.startswith("grad:") else FWD_TOL)
        if not v <= tol:
            bad[k] = v
    assert not bad, bad


def ralenet(variant, leads, L, B, sd, **kw):
    from ecg_denoise_amd import RALENet
    m = RALENet(variant, leads=leads, L=L, max_batch=B, train=True, device=DEV, **kw)
    m.load_state_dict(sd, strict=False)
    return m.freeze_bn().train()


def unet(leads, L, B, sd, **kw):
    from ecg_denoise_amd import UNet
    m = UNet(leads=leads, L=L, max_batch=B, device=DEV, **kw)
    m.load_state_dict(sd, strict=False)
    return m.freeze_bn().train()


def unet_case(leads, L, B, seed=1234):
    p32 = O.init_params(O.unet_param_shapes(leads), seed)
    g = torch.Generator().manual_seed(2023)
    return p32, torch.randn(B, leads, L, generator=g), torch.randn(B, leads, L, generator=g)


# ---- case 1: RA-LENet -------------------------------------------------------------------------------------------------
# 32: the smallest legal length; 320: padded token slots (Lp = 512); 256: a fast shape; both `leads` templates of the stem
@pytest.mark.parametrize("variant,leads,L,B", [("full", 2, 32, 3), ("nra", 1, 128, 5), ("mlp", 2, 320, 2), ("full", 2, 256, 3)])
def test_ralenet_frozen_step_matches_oracle(variant, leads, L, B):
    p32, x, tgt = make_case(variant, leads, L, B)
    sd, bns = with_statistics(p32)
    m = ralenet(variant, leads, L, B, sd)
    assert m.bn_frozen
    snap = snapshot(m)
    xd, td = x.to(DEV), tgt.to(DEV)
    y = m(xd)
    loss, _, _ = m.loss_and_metrics(y, td)
    m.backward()
    torch.cuda.synchronize()
    p, bn = oracle_leaves(sd, bns)
    xo = x.double().requires_grad_(True)
    yo = O.ralenet_forward(p, xo, variant, training=False, bn=bn)
    lo = O.mse(yo, tgt.double())
    *grads, dxo = torch.autograd.grad(lo, list(p.values()) + [xo], allow_unused=True)
    res = OrderedDict(y=rel(y.cpu().numpy(), yo.detach().numpy()), loss=abs(loss.item() - lo.item()) / abs(lo.item()))
    res.update(compare_grads(m.named_grads(), p, grads))
    assert len([k for k in res if k.startswith("grad")]) >= len(p)          # every parameter, the BatchNorm affines and tables too
    dx = m.backward(want_dx=True)                                           # ral_backward(dx): the stem stores dz as well
    torch.cuda.synchronize()
    res["grad:input"] = rel(dx.cpu().numpy(), dxo.numpy())
    stem = [k for k in p if k.startswith("conv1.")]
    again = compare_grads(m.named_grads(), OrderedDict((k, p[k]) for k in stem), [grads[list(p).index(k)] for k in stem])
    res.update((k + "@dx", v) for k, v in again.items())
    dxf = m.backward_input(m._dy)                                           # the chain NewRALE training runs
    torch.cuda.synchronize()
    res["grad:input_frozen"] = rel(dxf.cpu().numpy(), dxo.numpy())
    worst = max((v, k) for k, v in res.items() if k.startswith("grad:"))
    print(f"\nobserved {variant} {leads}x{L} B={B}: y {res['y']:.2e}, worst gradient {worst[0]:.2e} ({worst[1]})")
    check(res)
    assert_untouched(m, snap)
    assert (m.eng.bn_sums == 0).all(), "nothing is left in bn_sums"


# ---- case 2: U-Net ----------------------------------------------------------------------------------------------------
UNET_SHAPES = [(1, 48, 5), (2, 256, 3)]


def test_unet_shapes_run_the_generic_and_the_templated_stage_kernels():
    """(1, 48, 5): levels 24 / 12 / 6 / 3 - the stages whose lengths are no multiple of 4 run k_unet_fwd / k_unet_bwd, the outer
    ones the templated kernels; (2, 256, 3): templated kernels throughout, the fold of the weight-gradient partials"""
    fwd, bwd = set(), set()
    for leads, L, B in UNET_SHAPES:
        for si in range(11):
            fwd.add(query("train", leads, L, B, si)[0].split("<")[0])
            bwd.add(query("bwd", leads, L, B, si)[0].split("<")[0])
    assert fwd == {"k_unet_fwd", "k_unet_fwd_t"} and bwd == {"k_unet_bwd", "k_unet_bwd_t"}, (fwd, bwd)
    assert {query("bwd", leads, L, B, 0)[5] for leads, L, B in UNET_SHAPES} == {0, 1}       # with and without the fold


@pytest.mark.parametrize("leads,L,B", UNET_SHAPES)
@pytest.mark.parametrize("one_call", [False, True], ids=["forward+loss_means", "forward_loss_means"])
def test_unet_frozen_step_matches_oracle(leads, L, B, one_call):
    p32, x, tgt = unet_case(leads, L, B)
    sd, bns = with_statistics(p32)
    m = unet(leads, L, B, sd)
    snap = snapshot(m)
    xd, td = x.to(DEV), tgt.to(DEV)
    if one_call:                              # ral_forward_loss_means, then ral_backward(NULL)
        y, loss, _, _ = m.forward_loss(xd, td)
        assert m._dy_fused
        m.backward()
    else:                                     # ral_forward, ral_loss_means, ral_backward(dy)
        y = m(xd)
        loss, _, _ = m.loss_and_metrics(y, td)
        m.backward()
    torch.cuda.synchronize()
    p, bn = oracle_leaves(sd, bns)
    yo = O.unet_forward(p, x.double(), False, bn)
    lo = O.mse(yo, tgt.double())
    grads = torch.autograd.grad(lo, list(p.values()))
    res = OrderedDict(y=rel(y.cpu().numpy(), yo.detach().numpy()), loss=abs(loss.item() - lo.item()) / abs(lo.item()))
    ng = m.named_grads()
    for (k, _), g in zip(p.items(), grads):
        assert g.norm().item() > 1e-9, k      # (no structurally zero gradient under stored statistics: every key has a relative error)
        res["grad:" + k] = rel(ng[k].cpu().numpy(), g.numpy())
    assert len(grads) == len(ng) == 42
    worst = max((v, k) for k, v in res.items() if k.startswith("grad:"))
    wbias = max((v, k) for k, v in res.items() if k.endswith("conv.bias") or k in ("grad:bottleneck.0.bias", "grad:bottleneck.3.bias"))
    print(f"\nobserved U-Net {leads}x{L} B={B} one_call={one_call}: y {res['y']:.2e}, worst gradient {worst[0]:.2e} ({worst[1]}), "
          f"worst conv bias in front of a BatchNorm {wbias[0]:.2e} ({wbias[1]})")
    check(res)
    assert_untouched(m, snap)
    assert (m.eng.bn_sums == 0).all(), "nothing is left in bn_sums"


# ---- case 3: NewRALE ---------------------------------------------------------------------------------------------------
def test_newrale_frozen_adapter_step_matches_oracle():
    from ecg_denoise_amd import NewRALE, RALENet
    variant, L, B = "full", 32, 2
    p32, pa32, x, tgt = make_newrale_case(variant, L, B)
    sd, bns = with_statistics(p32)
    inner = RALENet(variant, leads=2, L=L, max_batch=B, train=True, device=DEV)
    inner.load_state_dict(sd, strict=False)
    m = NewRALE(inner, freeze_bn=True)
    m.load_state_dict(pa32)
    m.train()
    assert m.bn_frozen and inner.bn_frozen
    snap = snapshot(inner)
    inner_before = inner.eng.params.clone()
    y = m(x.to(DEV))
    loss, _, _ = m.loss_and_metrics(y, tgt.to(DEV))
    m.backward()
    torch.cuda.synchronize()
    p, bn = oracle_leaves(sd, bns)
    p = OrderedDict((k, v.detach()) for k, v in p.items())
    pa = OrderedDict((k, v.double().requires_grad_(True)) for k, v in pa32.items())
    yo = O.newrale_forward(pa, p, x.double(), variant, False, bn)
    lo = O.mse(yo, tgt.double())
    grads = torch.autograd.grad(lo, list(pa.values()))
    res = OrderedDict(y=rel(y.cpu().numpy(), yo.detach().numpy()), loss=abs(loss.item() - lo.item()) / abs(lo.item()))
    for (k, g), mine in zip(zip(pa, grads), m.named_grads().values()):
        res["grad:" + k] = rel(mine.cpu().numpy(), g.numpy())
    assert len(grads) == 8
    check(res)
    assert_untouched(inner, snap)
    assert torch.equal(inner.eng.params, inner_before)
    # the training-mode adapter now IS the model inference runs
    m.eval()
    ye = m(x.to(DEV))
    torch.cuda.synchronize()
    assert rel(ye.cpu().numpy(), y.cpu().numpy()) < FWD_TOL


# ---- case 4: invariants over three steps ------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["ralenet", "unet"])
def test_three_frozen_steps_leave_the_statistics_and_follow_the_oracle_trajectory(net):
    if net == "ralenet":
        variant, leads, L, B = "full", 2, 32, 3
        p32, x, tgt = make_case(variant, leads, L, B)
        sd, bns = with_statistics(p32)
        m = ralenet(variant, leads, L, B, sd)
        fwd = lambda bn: (lambda leaves, xx: O.ralenet_forward(leaves, xx, variant, False, bn))
    else:
        leads, L, B = 2, 64, 3
        p32, x, tgt = unet_case(leads, L, B)
        sd, bns = with_statistics(p32)
        m = unet(leads, L, B, sd)
        fwd = lambda bn: (lambda leaves, xx: O.unet_forward(leaves, xx, False, bn))
    xd, td = x.to(DEV), tgt.to(DEV)
    snap = snapshot(m)
    y_train = m(xd)
    y_eval = m.eval()(xd)
    m.train()
    assert m.bn_frozen, "freeze_bn survives eval() / train()"
    torch.cuda.synchronize()
    assert rel(y_train.cpu().numpy(), y_eval.cpu().numpy()) < FWD_TOL
    losses = [m.train_step(xd, td)["loss"].item() for _ in range(3)]
    assert_untouched(m, snap)
    p, bn = oracle_leaves(sd, bns)
    p = OrderedDict((k, v.detach().clone()) for k, v in p.items())
    am = OrderedDict((k, torch.zeros_like(v)) for k, v in p.items())
    av = OrderedDict((k, torch.zeros_like(v)) for k, v in p.items())
    want = [O.train_step(p, x.double(), tgt.double(), fwd(bn), am, av, i)["loss"].item() for i in (1, 2, 3)]
    print(f"\nobserved {net}: losses {losses} against {want}")
    np.testing.assert_allclose(losses, want, rtol=TRAJ_RTOL)
    m.load_state_dict(sd, strict=False)
    assert m.bn_frozen, "freeze_bn survives load_state_dict"


# ---- case 5: the data-parallel halves, global_windows = B ---------------------------------------------------------------
def _grads_close(got, want):
    for k in want:
        assert rel(got[k].cpu().numpy(), want[k].cpu().numpy()) <= SPLIT_TOL, k


def test_split_ralenet_frozen():
    from ecg_denoise_amd.model import _ptr, _stream
    L_, lib = _lib(), _lib().lib()
    variant, leads, L, B = "full", 2, 32, 3
    p32, x, tgt = make_case(variant, leads, L, B)
    sd, _ = with_statistics(p32)
    ref = ralenet(variant, leads, L, B, sd)
    xd, td = x.to(DEV), tgt.to(DEV)
    y_ref = ref(xd)
    ref.loss_and_metrics(y_ref, td)
    dy = ref._dy.clone()
    dx_ref = ref.backward(dy, want_dx=True)
    g_ref = {k: v.clone() for k, v in ref.named_grads().items()}
    m = ralenet(variant, leads, L, B, sd)
    m.eng.bn_sums.fill_(7.0)                   # (what a caller's buffer may hold: the library zeroes what it would have filled)
    y, dx, dx_in = torch.empty_like(xd), torch.empty_like(xd), torch.empty_like(xd)
    h = m.eng.h
    L_.check(lib.ral_forward_begin(h, _ptr(xd), B, _stream()))
    torch.cuda.synchronize()
    assert (m.eng.bn_sums[:32] == 0).all(), "the forward sums a data-parallel caller all-reduces are zeros"
    L_.check(lib.ral_forward_end(h, _ptr(y), B, B, _stream()))
    L_.check(lib.ral_backward_begin(h, _ptr(dy), B, _stream()))
    L_.check(lib.ral_backward_end(h, _ptr(dx), B, B, _stream()))
    torch.cuda.synchronize()
    assert (m.eng.bn_sums == 0).all()
    _grads_close(m.named_grads(), g_ref)
    assert rel(y.cpu().numpy(), y_ref.cpu().numpy()) <= FWD_TOL and rel(dx.cpu().numpy(), dx_ref.cpu().numpy()) <= SPLIT_TOL
    L_.check(lib.ral_backward_input_begin(h, _ptr(dy), B, _stream()))
    L_.check(lib.ral_backward_input_end(h, _ptr(dx_in), B, B, _stream()))
    torch.cuda.synchronize()
    assert rel(dx_in.cpu().numpy(), dx_ref.cpu().numpy()) <= SPLIT_TOL
    assert (m.eng.bn_sums == 0).all()


def test_split_unet_frozen():
    from ecg_denoise_amd.model import _ptr, _stream
    L_, lib = _lib(), _lib().lib()
    leads, L, B = 2, 64, 3
    p32, x, tgt = unet_case(leads, L, B)
    sd, _ = with_statistics(p32)
    ref = unet(leads, L, B, sd)
    xd, td = x.to(DEV), tgt.to(DEV)
    y_ref = ref(xd)
    ref.loss_and_metrics(y_ref, td)
    dy = ref._dy.clone()
    ref.backward(dy)
    g_ref = {k: v.clone() for k, v in ref.named_grads().items()}
    m = unet(leads, L, B, sd)
    m.eng.bn_sums.fill_(7.0)
    y, h = torch.empty_like(xd), m.eng.h
    for si in range(11):
        L_.check(lib.ral_unet_forward_stage(h, _ptr(xd), B, 1, si, B, _stream()))
        torch.cuda.synchronize()
        assert (m.eng.bn_sums == 0).all(), f"forward stage {si}"
    L_.check(lib.ral_unet_forward_finish(h, _ptr(y), B, 1, B, _stream()))
    L_.check(lib.ral_unet_backward_start(h, _ptr(dy), B, B, _stream()))
    for si in range(10, -1, -1):
        torch.cuda.synchronize()
        assert (m.eng.bn_sums == 0).all(), f"in front of backward stage {si}"
        L_.check(lib.ral_unet_backward_stage(h, B, si, B, _stream()))
    L_.check(lib.ral_unet_backward_finish(h, B, B, _stream()))
    torch.cuda.synchronize()
    assert (m.eng.bn_sums == 0).all()
    assert rel(y.cpu().numpy(), y_ref.cpu().numpy()) <= FWD_TOL
    _grads_close(m.named_grads(), g_ref)


# ---- case 6: the option itself ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["ralenet", "unet"])
def test_option_values_and_a_toggle_between_forward_and_backward(net):
    from ecg_denoise_amd import RalError
    L_ = _lib()
    if net == "ralenet":
        p32, x, tgt = make_case("full", 2, 32, 2)
        m = ralenet("full", 2, 32, 2, with_statistics(p32)[0])
    else:
        p32, x, tgt = unet_case(2, 64, 2)
        m = unet(2, 64, 2, with_statistics(p32)[0])
    xd, td = x.to(DEV), tgt.to(DEV)
    for bad in (2, -1):
        with pytest.raises(RalError, match="bn_frozen"):
            L_.check(L_.lib().ral_set_option(m.eng.h, b"bn_frozen", bad))
    assert m.bn_frozen
    for first in (True, False):                # frozen forward -> default backward, and the other way round
        m.freeze_bn(first)
        m.loss_and_metrics(m(xd), td)
        m.freeze_bn(not first)
        poison = m.eng.grads.fill_(3.0).clone()
        with pytest.raises(RalError, match="bn_frozen changed since the last forward"):
            m.backward()
        torch.cuda.synchronize()
        assert torch.equal(m.eng.grads, poison), "the refused backward launched nothing"
        out = m.train_step(xd, td)             # ... and the handle is usable
        assert np.isfinite(out["loss"].item())
    # an eval forward ignores the option, and its backward is refused with the text it always had
    m.freeze_bn(True).eval()
    m(xd)
    with pytest.raises(RalError, match="backward must follow a training forward: the last forward was an eval one"):
        m.backward(td)
    m.train()


@pytest.mark.parametrize("net", ["ralenet", "unet"])
def test_back_at_zero_a_step_has_the_bits_of_a_handle_that_never_saw_the_option(net):
    """Equal bits can only be asked for where the step itself is deterministic: RA-LENet "nra" 1 x 16 at B = 1 and the U-Net
    2 x 64 at B = 2 are (two untouched handles there: 0 differing words in the prediction, gradients, parameters and state,
    measured on an MI355X); "full" 2 x 32 at B = 1 is not - the float atomics of its R-wave table gradients leave 27 words
    of two untouched handles apart - so it cannot carry this check."""
    from ecg_denoise_amd import RALENet, UNet
    if net == "ralenet":
        p32, x, tgt = make_case("nra", 1, 16, 1)
        sd, _ = with_statistics(p32)
        a = RALENet("nra", leads=1, L=16, max_batch=1, device=DEV)
        b = ralenet("nra", 1, 16, 1, sd)
    else:
        p32, x, tgt = unet_case(2, 64, 2)
        sd, _ = with_statistics(p32)
        a = UNet(leads=2, L=64, max_batch=2, device=DEV)
        b = unet(2, 64, 2, sd)
    a.load_state_dict(sd, strict=False)
    xd, td = x.to(DEV), tgt.to(DEV)
    b.loss_and_metrics(b(xd), td)              # a frozen forward and backward, no optimiser step: parameters and state as loaded
    b.backward()
    b.freeze_bn(False)
    assert not b.bn_frozen
    ra, rb = a.train().train_step(xd, td), b.train_step(xd, td)
    torch.cuda.synchronize()
    assert torch.equal(ra["pred"], rb["pred"]) and torch.equal(ra["loss"], rb["loss"])
    assert torch.equal(a.eng.grads, b.eng.grads) and torch.equal(a.eng.params, b.eng.params)
    assert torch.equal(a.eng.state, b.eng.state) and a.eng.counters == b.eng.counters
    assert all(v == 1 for v in a.eng.counters.values())


@pytest.mark.parametrize("kind,leads,L", [("acdae", 2, 64), ("danet", 2, 32)])
def test_networks_without_the_option_answer_as_before(kind, leads, L):
    from ecg_denoise_amd import ACDAE, DANet, RalError
    L_ = _lib()
    m = ACDAE(L=L, max_batch=2, device=DEV) if kind == "acdae" else DANet(L=L, max_batch=2, device=DEV)
    for value in (0, 1, 2):
        with pytest.raises(RalError, match="no options for this handle"):
            L_.check(L_.lib().ral_set_option(m.eng.h, b"bn_frozen", value))
    if kind == "acdae":
        assert m.freeze_bn() is m and not m.bn_frozen
    else:
        with pytest.raises(RalError, match="not provided"):
            m.freeze_bn()
        assert m.freeze_bn(False) is m and not m.bn_frozen


# ---- case 7: the autograd shim ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["ralenet", "unet"])
def test_autograd_shim_with_frozen_statistics_takes_the_step_of_train_step(net):
    import torch.nn.functional as F
    if net == "ralenet":
        p32, x, tgt = make_case("full", 2, 32, 2)
        sd, _ = with_statistics(p32)
        a, b = ralenet("full", 2, 32, 2, sd, autograd=True), ralenet("full", 2, 32, 2, sd)
    else:
        p32, x, tgt = unet_case(2, 64, 2)
        sd, _ = with_statistics(p32)
        a, b = unet(2, 64, 2, sd, autograd=True), unet(2, 64, 2, sd)
    xd, td = x.to(DEV), tgt.to(DEV)
    snap = snapshot(a)
    opt = torch.optim.Adam(a.parameters(), lr=0.001)
    opt.zero_grad()
    pre = a(xd)
    assert pre.grad_fn is not None
    loss = F.mse_loss(pre, td)
    loss.backward()
    opt.step()
    fused = b.train_step(xd, td)
    torch.cuda.synchronize()
    np.testing.assert_allclose(loss.item(), fused["loss"].item(), rtol=LOOP_LOSS_RTOL)
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert rel(pa.detach().cpu().numpy(), pb.cpu().numpy()) < LOOP_PARAM_TOL, k
    assert_untouched(a, snap)
