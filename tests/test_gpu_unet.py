"""U-Net baseline (reference model/UNet.py) on the HIP path vs the oracle and the golden vectors.

Tolerances of the train-step test (fp32 kernels against the oracle in fp64, relative L2): one bar per tensor, 4 times the error of
that tensor in the oracle evaluated in fp32 (tests/parity_bars.py: the yardstick, floored at the median of its group -
the gradients, and everything else), never above the flat 1e-5 (forward) and 1e-4 (gradients) every case had before.  4, not the
8 of tests/test_gpu_parity.py: no U-Net kernel multiplies fp16 pairs.  A case gets such bars only if no LeakyReLU input is within
1e-5 of its tensor's RMS of 0 and fp32 and fp64 agree on every sign (the kink precondition, checked in
tests/test_baseline_bars_cpu.py).  The typical yardstick is 5e-8 (running statistics), 3e-7 (output) and 1e-6 (gradients).

Observed on an MI355X, as error over yardstick (with its floor; the bar is at 4): the worst tensor and the median per group
  case (leads, L, B) seed   forward: worst                       median   gradients: worst              median
  2, 512, 4     2023        1.83 loss                            0.54     2.72 DecList.3.conv.weight    0.81
  1, 256, 3     2023        1.00 DecList.2.bn.running_mean       0.65     1.03 EncList.1.bn.bias        0.66
  2, 1024, 2    2023        1.19 EncList.2.bn.running_mean       0.70     0.89 bottleneck.3.bias        0.62
  2, 48, 5      2024        1.19 EncList.1.bn.running_mean       0.76     0.92 DecList.2.bn.bias        0.35
  2, 320, 3     2023        1.00 DecList.3.bn.running_mean       0.75     1.46 DecList.2.bn.weight      0.69
(2, 48, 5) at seed 2023 and (2, 64, 1025) miss the precondition and keep the flat bars."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import baseline_parity_util as U
import ralenet_oracle as O
from parity_bars import check, errors
from parity_util import rel, run_unet, step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(leads, L, B, seed=1234):
    from ecg_denoise_amd import UNet
    p32 = O.init_params(O.unet_param_shapes(leads), seed)
    g = torch.Generator().manual_seed(2023)
    x = torch.randn(B, leads, L, generator=g); tgt = torch.randn(B, leads, L, generator=g)
    m = UNet(leads=leads, L=L, max_batch=B, device=DEV)
    m.load_state_dict(p32, strict=False)
    m.train()
    y = m(x.to(DEV))
    loss, snr, rmse = m.loss_and_metrics(y, tgt.to(DEV))
    m.backward()
    torch.cuda.synchronize()
    p = OrderedDict((k, v.double().requires_grad_(True)) for k, v in p32.items())
    bn = O.unet_bn_state(p, torch.float64)
    yo = O.unet_forward(p, x.double(), True, bn)
    lo = O.mse(yo, tgt.double())
    grads = torch.autograd.grad(lo, list(p.values()))
    return m, y, loss, p, bn, yo, lo, grads, x, tgt


# (2, 48, 5): a level length that is not a multiple of 4 -> generic stage kernels, gradient atomics instead of the fold;
# (2, 320, 3): fold path, stage-by-stage eval forward (the fused kernel takes multiples of 256 only);
# (2, 64, 1025): more windows than workgroup slots with a ragged last pass (1 window of 2), short levels (4 samples)
@pytest.mark.parametrize("case,seed,seeds", U.case_params("unet"))
def test_unet_train_step_matches_oracle(case, seed, seeds):
    """Output, loss, the running statistics of the ten BatchNorms, every parameter gradient and the eval forward after the step,
    each at its own bar: K_FP32 x what the fp32 oracle deviates from the fp64 one on that tensor, never above the flat 1e-5
    (forward) / 1e-4 (gradients) - baseline_parity_util.  (2, 48, 5) has a LeakyReLU input 2.4e-6 of its RMS from 0 at input
    seed 2023: it runs at seed 2024 under per-tensor bars and at 2023 under the flat ones.  (2, 64, 1025) has 2.4 million
    LeakyReLU inputs and no seed among nine keeps them all 1e-5 from 0: flat bars."""
    bars, yard = U.case_bars("unet", case, seed, seeds)
    mine, m = run_unet(case, seed, DEV)
    ref = step("unet", case, torch.float64, seed).vals
    check(errors(mine, ref), bars, yard, what="U-Net leads=%d L=%d B=%d seed %d" % (case + (seed,)))
    for k in O.UNET_BN:
        for s in (".running_mean", ".running_var"):
            np.testing.assert_allclose(mine[k + s], ref[k + s], rtol=1e-5, atol=1e-6)


def test_unet_against_reference_golden(golden_dir):
    from ecg_denoise_amd import UNet
    g = np.load(os.path.join(golden_dir, "g3_unet_l2_L512.npz"))
    p = O.init_params(O.unet_param_shapes(2), 1234)
    x = torch.tensor(g["x"]).to(DEV); tgt = torch.tensor(g["target"]).to(DEV)
    m = UNet(leads=2, L=512, max_batch=4, device=DEV)
    m.load_state_dict(p, strict=False)
    assert [k for k, _ in m.named_parameters()] == [str(k) for k in g["keys"]]
    m.train()
    y = m(x)
    assert rel(y.cpu().numpy(), g["y_train"]) < 1e-5
    loss, _, _ = m.loss_and_metrics(y, tgt)
    m.backward()
    ng = m.named_grads()
    keys = [str(k) for k in g["keys"]]
    gn = np.array([ng[k].double().norm().item() for k in keys])
    ok = g["grad_norm"] > 1e-5   # conv biases in front of a BatchNorm: exactly-zero gradient, rounding noise
    np.testing.assert_allclose(gn[ok], g["grad_norm"][ok], rtol=2e-4)
    m.eval()
    assert rel(m(x).cpu().numpy(), g["y_eval"]) < 1e-5
    m2 = UNet(leads=2, L=512, max_batch=4, device=DEV)
    m2.load_state_dict(p, strict=False)
    m2.train()
    losses = [m2.train_step(x, tgt)["loss"].item() for _ in range(3)]
    np.testing.assert_allclose(losses, g["adam_losses"], rtol=5e-4)


# (1024, 2048) and (2048, 1100): long windows at a full grid - the launchers cut the windows per pass to what two workgroups
# per CU leave of the LDS (32-channel stages at L = 2048: 64 KB for two windows), so a workgroup loops over several passes,
# the last one ragged at 1100 windows; the dynamic LDS above 64 KB is opted into per instantiation
@pytest.mark.parametrize("L,B", [(512, 2048), (1024, 2048), (2048, 1100)])
def test_unet_bench_batch_matches_fp64_oracle(L, B):
    """BASELINE batch (2048 x 2 x 512): every stage kernel runs its multi-window loop (512 workgroups), the wide layers'
    MFMA gradient products accumulate over four windows per workgroup, and the BatchNorm statistics are sums over 2048
    windows.  Output, loss and running statistics at the usual 1e-5; gradients at 1e-3 or 4 x what an fp32 evaluation of
    the oracle itself deviates by (LeakyReLU has a kink at 0: with 50-100 M activations a few sit within fp32 rounding of
    it and take the other slope in fp64)."""
    m, y, loss, p, bn, yo, lo, grads, x, tgt = _run(2, L, B, seed=4321)
    assert rel(y.cpu().numpy(), yo.detach().numpy()) < 1e-5
    assert abs(loss.item() - lo.item()) < 1e-5 * abs(lo.item())
    # what fp32 arithmetic itself costs at this size: the oracle evaluated in fp32 on the CPU against its fp64 evaluation
    # (2048 x 2 x 1024: 1.4e-3 .. 2.0e-3 on the encoder's gradients - twice the activations, twice the slope flips; the HIP
    # path measured 1.6e-3 .. 3.1e-3 there, tools/diag/unet_kink.py)
    p32 = OrderedDict((k, v.detach().float().requires_grad_(True)) for k, v in p.items())
    y32 = O.unet_forward(p32, x.float(), True, O.unet_bn_state(p32, torch.float32))
    g32 = torch.autograd.grad(O.mse(y32, tgt.float()), list(p32.values()))
    e32 = max(rel(gf.numpy(), gr.numpy()) for gf, gr in zip(g32, grads) if gr.norm().item() >= 1e-9)
    bound = max(1e-3, 4.0 * e32)     # (both deviations are sums of a few hundred slope flips: their ratio wanders between 1 and 3)
    ng = m.named_grads()
    bad = {}
    for (k, _), gr in zip(p.items(), grads):
        if gr.norm().item() < 1e-9:                   # zero gradient in front of a batch-statistics BatchNorm
            if float(np.abs(ng[k].cpu().numpy()).max()) > 2e-5:
                bad[k] = "nonzero"
            continue
        e = rel(ng[k].cpu().numpy(), gr.numpy())
        # the last layer's gradients see no LeakyReLU on the way back (DecList.3 is ConvTranspose1d + BatchNorm, then the loss):
        # no slope can flip between fp32 and fp64, so they keep the tight bar whatever the size - a regression of a few 1e-3
        # in the MFMA conv / weight-gradient paths cannot hide behind the kink allowance of the other layers
        if e > (2e-4 if k.startswith("DecList.3.") else bound):
            bad[k] = e
    assert not bad, (bad, bound)
    sd = m.state_dict()
    for k in O.UNET_BN:
        np.testing.assert_allclose(sd[k + ".running_mean"].cpu().numpy(), bn[k]["running_mean"].numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(sd[k + ".running_var"].cpu().numpy(), bn[k]["running_var"].numpy(), rtol=1e-5, atol=1e-6)


def test_unet_backward_twice_gives_the_same_gradients():
    """two backward passes after one forward (replica records and scratch rows are re-initialised per pass): the gradients
    agree to the rounding noise of the in-kernel float atomics (LDS sums of position splits, BatchNorm-backward sums)"""
    from ecg_denoise_amd import UNet
    B, L = 1024, 512
    m = UNet(leads=2, L=L, max_batch=B, device=DEV, seed=5)
    x = torch.randn(B, 2, L, device=DEV); t = torch.randn(B, 2, L, device=DEV)
    m.train()
    y = m(x); m.loss_and_metrics(y, t)
    m.backward(); g1 = {k: v.clone() for k, v in m.named_grads().items()}
    m.backward(); g2 = m.named_grads()
    for k in g1:
        if g1[k].double().norm().item() > 1e-7:          # (zero-gradient biases in front of a BatchNorm are pure noise)
            assert rel(g2[k].cpu().numpy(), g1[k].cpu().numpy()) < 1e-5, k


def test_unet_refuses_an_input_gradient():
    """the U-Net forms no input gradient: `backward(want_dx=True)` is refused, not answered with an unwritten tensor"""
    from ecg_denoise_amd import RalError, UNet
    m = UNet(leads=2, L=64, max_batch=2, device=DEV, seed=5)
    x = torch.randn(2, 2, 64, device=DEV)
    m.train()
    m.loss_and_metrics(m(x), torch.zeros_like(x))
    with pytest.raises(RalError, match="U-Net input gradient is not provided"):
        m.backward(want_dx=True)
    m.backward()                                      # (the refusal leaves the saved forward usable)
    torch.cuda.synchronize()


@pytest.mark.parametrize("leads,L,B", [(2, 512, 2048), (1, 256, 37), (2, 48, 5), (2, 2048, 9), (2, 64, 1025)])
def test_unet_forward_loss_in_one_call_equals_forward_then_loss(leads, L, B):
    """`forward_loss` (ral_forward_loss_means: the output BatchNorm, the loss sums, dy and the first two sums of the backward pass
    in ONE kernel, k_unet_out_loss) against `forward` + `loss_and_metrics` + `backward` (k_unet_out, k_loss_w, k_unet_gsums) on
    twin models: the prediction, dy, the per-window metrics and the loss to 1e-6, the running
    statistics and every gradient to the rounding noise of the atomics.  Then a second backward from the same dy (the sums of
    the one-call path are used once; the second pass forms them with k_unet_gsums) and a backward from a COPY of dy (another
    pointer: the sums left behind must not be used)."""
    from ecg_denoise_amd import UNet
    p32 = O.init_params(O.unet_param_shapes(leads), 77)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, leads, L, generator=g).to(DEV); t = torch.randn(B, leads, L, generator=g).to(DEV)
    a = UNet(leads=leads, L=L, max_batch=B, device=DEV); a.load_state_dict(p32, strict=False); a.train()
    b = UNet(leads=leads, L=L, max_batch=B, device=DEV); b.load_state_dict(p32, strict=False); b.train()
    ya = a(x); la, sa, ra = a.loss_and_metrics(ya, t); a.backward()
    yb, lb, sb, rb = b.forward_loss(x, t); b.backward()
    torch.cuda.synchronize()
    # (twin models: their BatchNorm sums are accumulated with atomics in an order of their own - equal to rounding, not bit for bit)
    assert rel(yb.cpu().numpy(), ya.cpu().numpy()) < 1e-6 and rel(b._dy.cpu().numpy(), a._dy.cpu().numpy()) < 1e-6
    # (the sums of squares are the same expressions in two kernels, contracted into fused multiply-adds as the compiler saw fit in each)
    assert rel(sb.cpu().numpy(), sa.cpu().numpy()) < 1e-6 and rel(rb.cpu().numpy(), ra.cpu().numpy()) < 1e-6
    assert abs(la.item() - lb.item()) <= 1e-6 * abs(la.item())
    ga, gb = a.named_grads(), b.named_grads()

    def same(g1, g2):
        for k in g1:
            if g1[k].double().norm().item() > 1e-5:      # (the oracle bar of these gradients is 1e-4; two runs differ by the
                assert rel(g2[k].cpu().numpy(), g1[k].cpu().numpy()) < 5e-5, k   # noise of their float atomics, ~1e-5 on the BatchNorm weights)
    same(ga, gb)
    sda, sdb = a.state_dict(), b.state_dict()
    for k in sda:
        if "running" in k:
            np.testing.assert_allclose(sdb[k].cpu().numpy(), sda[k].cpu().numpy(), rtol=1e-6, atol=1e-7, err_msg=k)
    ref = {k: v.clone() for k, v in gb.items()}
    b.backward(); same(ref, b.named_grads())                     # the same dy again: k_unet_gsums this time
    yb2, _, _, _ = b.forward_loss(x, t)
    b.backward(b._dy.clone()); same(ref, b.named_grads())        # running statistics moved, batch statistics did not
