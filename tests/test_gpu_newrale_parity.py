"""A whole train step of the 12-lead adapter (reference model/ralenet_12leads.py::newrale: Conv1d 12->6->2, the frozen 2-lead
RA-LENet, Conv1d 2->6->12) against the fp64 oracle, and three Adam steps against O.train_step / O.adam_step.

The cases are the smallest at which each thing can still go wrong:
  ("full", 256, 3)   the plain case
  ("nra", 16, 4)     the 13-tap halo (6) against L = 16; one token at the deep levels; n = 192: n / 4 < 64 lanes of the loss
  ("full", 32, 2)    the smallest length with R-wave tables
  ("mlp", 320, 2)    Lp = 512 > L: the zero fill of dz and the tap guard of the stem's input gradient, on the frozen chain
  ("nra", 64, 5)     an odd batch
  ("full", 1008, 1)  one tile short of 1024
  ("nra", 16, 513)   k_conv13_bwd beyond its 512 workgroups (workgroup 0 takes two windows, the others one); the inner model
                     at a batch above 512

Bars of the train step: one per quantity, 4 times its error in the oracle evaluated in fp32 (tests/parity_bars.py: the
yardstick, floored at the median of its group), never above the flat forward 1e-5 and gradients 1e-4 of tests/parity_bars.py;
4, since the adapter's own kernels multiply no fp16 pairs and the frozen inner model's forward sits at the fp32 oracle's error
(tests/test_gpu_parity.py).  A case gets them only if no input of the three adapter LeakyReLUs and of the stem's is within 1e-5 of
its tensor's RMS of 0 (tests/test_baseline_bars_cpu.py): ("nra", 64, 5) moves to input seed 2024 for that and runs at 2023 under
the flat bars, ("nra", 16, 513) keeps the flat bars.  The Adam trajectory: the bars of tests/test_gpu_danet.py (2e-5 on the
prediction after a step, 1e-5 on the parameters after the last).  The fp64 oracle evaluated in fp32 differs from itself by up to
4.9e-7 on y and 1.2e-6 on the adapter gradients.

Observed on an MI355X, as error over yardstick (with its floor; the bar is at 4): the worst quantity and the median per group
  case               forward: worst   median   gradients: worst    median
  full, 256, 3       1.16 y_eval      0.54     2.64 conv1.bias     0.74
  nra, 16, 4         1.12 y           0.63     1.16 conv3.weight   0.85
  full, 32, 2        1.57 y           0.69     2.21 conv2.bias     1.55
  mlp, 320, 2        1.06 y           0.41     0.89 conv1.weight   0.57
  nra, 64, 5 @2024   1.13 y_eval      0.75     1.24 conv1.weight   0.80
  full, 1008, 1      2.03 snr         0.31     3.12 conv2.bias     1.49

Observed worst errors on an MI355X (train step: forward = max over y, loss, SNR, RMSE, BatchNorm statistics, y_eval):
  case               forward (which)   y        y_eval   gradient (which)       | Adam: loss   prediction  parameters
  full, 256, 3       2.3e-6 (snr)      4.5e-7   2.8e-7   1.8e-6 (conv1.bias)    |       2.3e-8  5.0e-7      6.9e-8
  nra, 16, 4         1.4e-6 (snr)      5.7e-7   2.7e-7   5.8e-7 (conv3.weight)  |       8.8e-8  7.2e-7      5.6e-8
  full, 32, 2        3.8e-6 (snr)      6.6e-7   2.6e-7   1.3e-6 (conv2.bias)    |       5.6e-8  6.6e-7      1.7e-7
  mlp, 320, 2        3.2e-6 (snr)      5.3e-7   4.2e-7   8.4e-7 (conv1.bias)    |       2.7e-8  6.2e-7      6.8e-8
  nra, 64, 5         1.6e-6 (snr)      4.5e-7   3.1e-7   8.9e-7 (conv1.bias)    |       2.9e-8  5.2e-7      6.5e-8
  full, 1008, 1      5.5e-6 (snr)      4.6e-7   2.7e-7   1.5e-6 (conv2.bias)    |       3.9e-8  5.0e-7      9.3e-8
  nra, 16, 513       1.5e-6 (snr)      4.1e-7   3.0e-7   2.6e-6 (conv1.bias)    |       6.7e-9  4.3e-7      6.5e-8
(the SNR leads the forward column because a window's SNR is -0.06 .. -0.17 dB here - unit-variance target, loss 1.01 .. 1.04 -
and the fp32 rounding of the ratio, 6e-8, is divided by it)."""
import pytest
import torch

import baseline_parity_util as U
from parity_bars import FWD_TOL, GRAD_TOL, check
from parity_util import run_newrale_adam, run_newrale_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = [("full", 256, 3), ("nra", 16, 4), ("full", 32, 2), ("mlp", 320, 2), ("nra", 64, 5), ("full", 1008, 1), ("nra", 16, 513)]
ADAM_PRED_TOL, ADAM_PARAM_TOL = 2e-5, 1e-5     # tests/test_gpu_danet.py


@pytest.mark.parametrize("case,seed,seeds", U.case_params("newrale"))
def test_adapter_train_step_matches_oracle(case, seed, seeds):
    """Every quantity of run_newrale_parity at its own bar: K_FP32 x what the fp32 oracle deviates from the fp64 one on it, never
    above the flat bars (baseline_parity_util).  ("nra", 64, 5) has an adapter LeakyReLU input 8.2e-6 of its RMS from 0 at input
    seed 2023: per-tensor bars at seed 2024, the flat ones at 2023.  ("nra", 16, 513) has 361 000 LeakyReLU inputs and no seed
    among nine keeps them all 1e-5 from 0: flat bars."""
    variant, L, B = case
    assert case in CASES
    res = run_newrale_parity(variant, L, B, DEV, seed)
    fwd = {k: v for k, v in res.items() if not k.startswith("grad:")}
    grad = {k: v for k, v in res.items() if k.startswith("grad:")}
    kf, kg = max(fwd, key=fwd.get), max(grad, key=grad.get)
    print(f"\nobserved {variant} L={L} B={B}: forward {fwd[kf]:.2e} ({kf}), y {res['y']:.2e}, y_eval {res['y_eval']:.2e}, "
          f"gradient {grad[kg]:.2e} ({kg})")
    assert len(grad) == 8
    bars, yard = U.case_bars("newrale", case, seed, seeds)
    check(res, bars, yard, what=f"adapter {variant} L={L} B={B} seed {seed}")


@pytest.mark.parametrize("variant,L,B", CASES)
def test_adapter_adam_trajectory_matches_oracle(variant, L, B):
    res, m, inner_before = run_newrale_adam(variant, L, B, 3, DEV)
    worst = lambda pre: max(v for k, v in res.items() if k.startswith(pre))
    print(f"\nobserved {variant} L={L} B={B}: loss {worst('loss'):.2e}, prediction {worst('pred'):.2e}, parameters {worst('param:'):.2e}")
    bad = {}
    for k, v in res.items():
        # step 1 runs on the initial parameters: the forward bar; later steps and the parameters: the DANet test's bars
        tol = ADAM_PARAM_TOL if k.startswith("param:") else (FWD_TOL if k.endswith("1") else ADAM_PRED_TOL)
        if not v <= tol:
            bad[k] = v
    assert not bad, bad
    assert torch.equal(inner_before, m.rale.eng.params)               # frozen inner weights, bit for bit
    assert m.step_count == 3 and m.rale.step_count == 0
    # tensors start on multiples of 4 floats: the floats between them belong to no tensor and stay zero under Adam
    used = torch.zeros(m.params.numel(), dtype=torch.bool)
    for k, shp in m.SHAPES.items():
        used[m.off[k]:m.off[k] + int(torch.tensor(shp).prod())] = True
    assert (~used).sum().item() == 6 and used.sum().item() == 2210
    assert torch.equal(m.params.cpu()[~used], torch.zeros(6))


def test_adapter_refuses_an_input_gradient():
    from ecg_denoise_amd import NewRALE, RALENet, RalError
    m = NewRALE(RALENet("nra", leads=2, L=16, max_batch=1, device=DEV, seed=1), seed=2)
    dy = torch.zeros(1, 12, 16, device=DEV)
    with pytest.raises(RalError, match="input gradient is not provided"):
        m._backward_raw(dy, want_dx=True)
    assert GRAD_TOL == 1e-4 and FWD_TOL == 1e-5                       # the bars this file borrows
