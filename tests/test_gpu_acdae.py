"""ACDAE comparison baseline (reference model/ACDAE.py) on the HIP path vs the fp64 oracle and the reference's golden
vectors: outputs, loss, every parameter gradient, the input gradient, three Adam steps.

Tolerances of the train-step test (fp32 kernels against the oracle in fp64, relative L2): one bar per tensor, 4 times the error of
that tensor in the oracle evaluated in fp32 (tests/parity_bars.py: the yardstick, floored at the median of its group),
never above the flat 1e-5 (forward) and 1e-4 (gradients) every case had before.  A case gets such bars only if no LeakyReLU input
and no MaxPool1d(2) pair is within 1e-5 of its tensor's RMS of its kink and fp32 and fp64 agree on every one (the kink
precondition, tests/test_baseline_bars_cpu.py).  The typical yardstick is 3e-7, so the typical bar 1.2e-6 where it was 1e-4: the
ECA gate's sigmoid on the fast exponential (k_acd_dec_fwd) stays within it, 1.44 x the yardstick at most on an ECA weight gradient.

Observed on an MI355X, as error over yardstick (with its floor; the bar is at 4): the worst tensor and the median per group
  case (L, B) seed   forward: worst   median   gradients: worst                median
  512, 4    2025     1.24 y           0.64     1.44 DecList.1.ECA.conv.weight  0.65
  256, 3    2023     1.20 y           0.67     1.22 EncList.3.conv.weight      0.83
  1024, 2   2026     1.21 y           0.61     1.08 input                      0.45
  64, 3     2023     1.11 y           0.62     0.95 DecList.1.ECA.conv.weight  0.46
  192, 2    2023     1.22 y           0.62     2.18 DecList.2.conv.bias        1.69
(512, 4) and (1024, 2) at seed 2023 miss the precondition and keep the flat bars."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import baseline_parity_util as U
import ralenet_oracle as O
from parity_bars import check, errors
from parity_util import rel, run_acdae, step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("case,seed,seeds", U.case_params("acdae"))
def test_acdae_train_step_matches_oracle(case, seed, seeds):
    """Output, loss, every parameter gradient and the input gradient, each at its own bar: K_FP32 x what the fp32 oracle
    deviates from the fp64 one on that tensor, never above the flat 1e-5 / 1e-4 (baseline_parity_util).  (512, 4) and (1024, 2)
    have a LeakyReLU input 9.0e-6 / 4.9e-6 of its RMS from 0 at input seed 2023: they run at seeds 2025 / 2026 under
    per-tensor bars and at 2023 under the flat ones.  The per-window SNR keeps its absolute 1e-4 (it is near 0 dB here: a relative
    error says little), eval against train mode its bit equality."""
    bars, yard = U.case_bars("acdae", case, seed, seeds)
    mine, m, x, y, snr, tgt = run_acdae(case, seed, DEV)
    o = step("acdae", case, torch.float64, seed)
    check(errors(mine, o.vals), bars, yard, what="ACDAE L=%d B=%d seed %d" % (case + (seed,)))
    yo = torch.from_numpy(o.vals["y"])
    np.testing.assert_allclose(snr.cpu().numpy(), O.snr(tgt.double(), yo).numpy(), rtol=0, atol=1e-4)
    m.eval()
    assert torch.equal(m(x.to(DEV)), y)                    # no BatchNorm, no dropout: eval is the same function


def test_acdae_against_reference_golden(golden_dir):
    from ecg_denoise_amd import ACDAE
    g = np.load(os.path.join(golden_dir, "g3_acdae_l2_L512.npz"))
    p = O.init_params(O.acdae_param_shapes(), 1234)
    x = torch.tensor(g["x"]).to(DEV); tgt = torch.tensor(g["target"]).to(DEV)
    m = ACDAE(L=512, max_batch=x.shape[0], device=DEV)
    assert [k for k, _ in m.named_parameters()] == [str(k) for k in g["keys"]]      # the reference's state_dict order
    m.load_state_dict(p)
    m.train()
    y = m(x)
    loss, _, _ = m.loss_and_metrics(y, tgt)
    m.backward()
    assert rel(y.cpu().numpy(), g["y_train"]) < 1e-5
    assert abs(loss.item() - g["loss"]) < 1e-5 * abs(g["loss"])
    ng = m.named_grads()
    gn = np.array([ng[str(k)].double().norm().item() for k in g["keys"]])
    np.testing.assert_allclose(gn, g["grad_norm"], rtol=2e-4, atol=1e-8)
    m2 = ACDAE(L=512, max_batch=x.shape[0], device=DEV)
    m2.load_state_dict(p)
    losses = [m2.train_step(x, tgt)["loss"].item() for _ in range(3)]
    np.testing.assert_allclose(losses, g["adam_losses"], rtol=5e-4)
    sd = m2.state_dict()
    assert list(sd) == [str(k) for k in g["keys"]] and sd["DecList.0.ECA.conv.weight"].shape == (1, 1, 3)


def test_acdae_trains_through_the_harness(tmp_path):
    """main.py:66-68 path: ACDAE through the same train() harness as the other models; the loss goes down"""
    from ecg_denoise_amd import ACDAE, synth
    from ecg_denoise_amd.train import train
    noisy, clean = synth.make_dataset(96, 2, 256, "emb", 0.0, seed=5)
    bat = lambda a, b, bs: [(a[i:i + bs], b[i:i + bs]) for i in range(0, len(a), bs)]
    m = ACDAE(L=256, max_batch=32, device=DEV, seed=3)
    res = train(epochs=10, model=m, batch_size=32, train_loader=bat(noisy[:64], clean[:64], 32), test_loader=bat(noisy[64:], clean[64:], 32),
                use_gpu=True, model_name="ACDAE", noise_name="emb", noise_intensity=0, out_dir=str(tmp_path), log=lambda *_: None)
    tl, _ = train.last_losses
    assert tl[-1] < tl[0] and all(np.isfinite(res[1]))
    assert (tmp_path / "model_save" / "ACDAE" / "ACDAE_9_emb_intensity0.pth").exists()


def test_acdae_bench_batch_is_the_sum_of_its_halves():
    """BASELINE batch (2048 x 2 x 512).  ACDAE has no BatchNorm, so windows are independent: the forward of a slice is the
    slice of the forward bit for bit, the input gradient likewise, and the parameter gradients of the whole batch are the
    sum of the gradients of its two halves (same upstream gradient) - which exercises the multi-window loops and the
    split-K accumulation of the MFMA weight-gradient kernel at full size.  64 windows of it also against the fp64 oracle."""
    from ecg_denoise_amd import ACDAE
    B, L = 2048, 512
    p32 = O.init_params(O.acdae_param_shapes(), 77)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, 2, L, generator=g).to(DEV)
    dy = (torch.randn(B, 2, L, generator=g) / (B * 2 * L)).to(DEV)
    m = ACDAE(L=L, max_batch=B, device=DEV); m.load_state_dict(p32); m.train()
    y = m(x).clone()
    dx = m.backward(dy, want_dx=True).clone()
    gw = OrderedDict((k, v.clone()) for k, v in m.named_grads().items())
    h = ACDAE(L=L, max_batch=B // 2, device=DEV); h.load_state_dict(p32); h.train()
    parts = []
    for lo in (0, B // 2):
        yh = h(x[lo:lo + B // 2].contiguous())
        assert torch.equal(yh, y[lo:lo + B // 2])
        dxh = h.backward(dy[lo:lo + B // 2].contiguous(), want_dx=True)
        assert torch.equal(dxh, dx[lo:lo + B // 2])
        parts.append(OrderedDict((k, v.clone()) for k, v in h.named_grads().items()))
    for k in gw:
        s2 = parts[0][k].double() + parts[1][k].double()
        assert rel(gw[k].double().cpu().numpy(), s2.cpu().numpy()) < 2e-5, k      # (fp32 atomics: the order of a million-term sum)
    # a slice against the oracle
    n = 64
    p = OrderedDict((k, v.double()) for k, v in p32.items())
    yo = O.acdae_forward(p, x[:n].cpu().double())
    assert rel(y[:n].cpu().numpy(), yo.numpy()) < 1e-5
