"""The Linear-layer kernel instances that a model can launch but no parity test of tests/test_gpu_parity.py or
tests/test_gpu_configs.py reaches, each against the fp64 oracle.  Needs an MI355X: `pytest -m gpu`.

tests/test_block_plan_cpu.py shows that the plan (csrc/ral_block_plan.hip) chooses every enumerator of BLOCK_KERNELS somewhere;
tests/test_block_coverage_cpu.py (the ledger) counts which of them a model can launch and which of those a GPU test compares with
the oracle.  The ones the other files leave are here:

  * the whole C = 32 split-operand family of f16_split = 32: k_qkv_fwd_h<32, 64>, k_mlp_fwd_h<32, 1 | 2 | 4, 512>, k_qkv_bwd_h<32> -
    and, once FUSE_DW < 32 takes C = 32 out of the fused backward, k_mlp_bwd_h<32, 1, 512>, k_mlp_bwd_h<32, 4, 256> and the four split
    weight-gradient products k_dw<..., true> of C = 32;
  * k_mlp_bwd<8, 1> and k_mlp_bwd<16, 1>: the unfused fp32 backward of the narrow levels at L = 256 (FUSE_DW = 0, 8);
  * f16_split = 128 (no instance of its own; C = 64 on fp32 with fp32 weight gradients beside C = 128 on pairs);
  * k_mlp_fwd_w<8 | 16 | 32>, the fp32 strip forward, in eval mode (MLP_FWD_W = 2; the parity tests run it in training only).

Every case is a whole train step (outputs, loss, metrics, BatchNorm statistics, every block output, every parameter gradient) and
the eval-mode forward of the same model, through parity_util.run_parity, at the bars of tests/test_gpu_parity.py: per tensor 8 times
its error in the fp32 oracle (parity_bars.yardstick), never above forward 1e-5 and gradients 1e-4; the key-bias half 1e-5
absolute.  The two `-spread` twins run the same instances with the fc1 biases a grid over [-9, 9] (parity_util.spread_fc1_bias),
in every process their originals run in: every MLP forward and backward family - k_mlp_fwd_h, k_mlp_fwd_w, the fused strips,
k_mlp_bwd, k_mlp_bwd_h - evaluates its GELU and the GELU's derivative across [-10, 10], not only below 3.  Before its forward a case asks ral_block_plan - same process, same switches -
whether the instances it exists for are in the plan of its model, so a case that stops reaching its kernel fails here too.  B is odd
where a level packs two windows into a 64-token group: the ragged last group is on the path.  FUSE_DW and MLP_FWD_W latch at their first read, so
the cases that need them run in a pytest process of their own (RAL_TEST_OPTIONS, tests/conftest.py).

Observed on an MI355X, per case and process (forward: the worst of output, eval output, loss, metrics, BatchNorm statistics
and the eighteen block outputs; gradient: the worst relative L2 over the parameter gradients):

  case                   process                  forward   gradient
  full-L256-B3-split32   default switches         4.0e-7    2.5e-6
  full-L256-B3-split32   f16_split=32,fuse_dw=0   3.9e-7    2.1e-6
  full-L256-B3-split32   f16_split=32,fuse_dw=16  4.0e-7    2.4e-6
  full-L512-B3-split32   default switches         3.9e-7    1.4e-6
  full-L512-B3-split32   f16_split=32,fuse_dw=0   3.8e-7    1.2e-6
  full-L512-B3-split32   f16_split=32,fuse_dw=16  3.9e-7    1.4e-6
  full-L768-B2-split32   default switches         4.2e-7    2.5e-6
  mlp-L256-B3-split32    default switches         4.0e-7    1.1e-6
  mlp-L256-B3-split32    f16_split=32,fuse_dw=0   4.0e-7    1.2e-6
  full-L512-B3-split128  default switches         3.9e-7    1.3e-6
  full-L256-B3-split64   default switches         3.9e-7    1.8e-6
  full-L256-B3-split64   fuse_dw=0                4.0e-7    1.8e-6
  full-L256-B3-split64   fuse_dw=8                4.0e-7    2.1e-6
  full-L256-B3-split64   mlp_fwd_w=2              6.9e-7    2.2e-6

The worst forward figure is a block output each time (the model output: 1.7e-7 .. 3.1e-7, eval 2.0e-7 .. 3.6e-7); the C = 32 pair
path sits where the default path does (tests/test_gpu_parity.py: 2e-7 / 2e-6).  Over the per-tensor yardstick (the table of
tests/test_gpu_parity.py explains the columns) the worst tensor of these cases, in every process, is at 1.0 .. 2.3 in the forward
group (2.3: blk5.out under mlp_fwd_w=2) and at 1.8 .. 3.6 among the gradients - in the twins at 3.8 .. 7.2, an attention query
gradient of dtransformer2.1 or dtransformer3.0 each time (7.2: f16_split=32,fuse_dw=0) - the medians at 0.7 .. 1.6 and
0.9 .. 1.6, where the bar is 8."""
import os
import subprocess
import sys

import pytest

from parity_bars import bars, check
from parity_util import parity_yardstick, run_parity, spread_fc1_bias
from test_block_plan_cpu import DW, MB, MBH, MFH, MFW, QBH, QH, model_instances

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_DW32H = [name % "true" for name in DW[32]]
_C32_BWD_256 = [MBH % (32, 1, 512)] + _DW32H          # (32, 64) off the fused backward: eight waves, split products
_C32_BWD_512 = [MBH % (32, 4, 256)] + _DW32H          # (32, 128): four waves

_SPLIT32_256 = {"": [QH % 32, MFH % (32, 1, 512), QBH % 32], "f16_split=32,fuse_dw=0": _C32_BWD_256, "f16_split=32,fuse_dw=16": _C32_BWD_256}
_SPLIT64_256 = {"fuse_dw=0": [MB % (8, 1), MB % (16, 1)], "fuse_dw=8": [MB % (16, 1)], "mlp_fwd_w=2": [MFW % 8, MFW % 16, MFW % 32]}

# (variant, L, B, f16_split, {option string of the process: the instances the case exists for under it}, spread: the fc1 biases a
# grid over [-9, 9] - parity_util.spread_fc1_bias)
CASES = [
    pytest.param("full", 256, 3, 32, _SPLIT32_256, False, id="full-L256-B3-split32"),
    pytest.param("full", 512, 3, 32, {"": [MFH % (32, 2, 512)],
                                      "f16_split=32,fuse_dw=0": _C32_BWD_512, "f16_split=32,fuse_dw=16": _C32_BWD_512}, False, id="full-L512-B3-split32"),
    pytest.param("full", 768, 2, 32, {"": [MFH % (32, 4, 512)]}, False, id="full-L768-B2-split32"),       # level (32, 192), training too
    pytest.param("mlp", 256, 3, 32, {"f16_split=32,fuse_dw=0": _C32_BWD_256}, False, id="mlp-L256-B3-split32"),   # no local-enhancement conv
    pytest.param("full", 512, 3, 128, {}, False, id="full-L512-B3-split128"),
    pytest.param("full", 256, 3, 64, _SPLIT64_256, False, id="full-L256-B3-split64"),
    # the twins: the same instances with GELU arguments across [-10, 10]
    pytest.param("full", 256, 3, 32, _SPLIT32_256, True, id="full-L256-B3-split32-spread"),
    pytest.param("full", 256, 3, 64, _SPLIT64_256, True, id="full-L256-B3-split64-spread"),
]
# the processes with latched switches: (option string, ids of the cases above it runs)
_S32, _S64 = "full-L256-B3-split32-spread", "full-L256-B3-split64-spread"
SWITCH_RUNS = [
    ("f16_split=32,fuse_dw=0", ("full-L256-B3-split32", "full-L512-B3-split32", "mlp-L256-B3-split32", _S32)),
    ("f16_split=32,fuse_dw=16", ("full-L256-B3-split32", "full-L512-B3-split32", _S32)),    # ... beside fused C = 8 / 16 strips
    ("fuse_dw=0", ("full-L256-B3-split64", _S64)),
    ("fuse_dw=8", ("full-L256-B3-split64", _S64)),
    ("mlp_fwd_w=2", ("full-L256-B3-split64", _S64)),      # the fp32 strips in eval mode (the parity tests run them in training only)
]
NARROW_F16 = 1            # the model's default; no case changes it


@pytest.mark.parametrize("variant,L,B,f16_split,names,spread", CASES)
def test_block_instances_match_oracle(variant, L, B, f16_split, names, spread):
    opts = os.environ.get("RAL_TEST_OPTIONS", "")
    want = set(names.get(opts, ()))
    forward = {n for n in want if n.startswith(("k_qkv_fwd", "k_mlp_fwd"))}

    def planned(model):
        train, evalm = (model_instances(L, mode, f16_split, NARROW_F16) for mode in (1, 0))
        assert want <= train and forward <= evalm, (opts, sorted(want - train), sorted(forward - evalm))

    params = spread_fc1_bias if spread else None
    res, _, _ = run_parity(variant, 2, L, B, DEV, options={"f16_split": f16_split}, eval_forward=True, before_forward=planned, params=params)
    fwd = {k: v for k, v in res.items() if not k.startswith(("grad:", "gradabs:"))}
    grad = {k: v for k, v in res.items() if k.startswith("grad:")}
    kf, kg = max(fwd, key=fwd.get), max(grad, key=grad.get)
    what = f"[{opts or 'default'}] {variant} L={L} B={B} f16_split={f16_split}{' spread' if spread else ''}"
    print(f"\nobserved {what}: forward {fwd[kf]:.2e} ({kf}), "
          f"y {res['y']:.2e}, y_eval {res['y_eval']:.2e}, gradient {grad[kg]:.2e} ({kg})")
    # a twin never had flat bars: 8 x each tensor's fp32-oracle error alone (its ill-conditioned query gradients are above 1e-4
    # in the fp32 oracle itself)
    yard = parity_yardstick(variant, 2, L, B, params=params, eval_forward=True)
    check(res, bars(yard, capped=not spread), yard, what=what)


@pytest.mark.parametrize("opts,ids", SWITCH_RUNS, ids=[opts for opts, _ in SWITCH_RUNS])
def test_block_instances_under_latched_switches(opts, ids):
    """the cases above that need a switch of the plan, in a process that sets it before the library's first use"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s", "-m", "gpu", "-k",
                        "test_block_instances_match_oracle and (%s)" % " or ".join(ids)],
                       env=dict(os.environ, RAL_TEST_OPTIONS=opts), cwd=root, capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert "%d passed" % len(ids) in p.stdout, p.stdout[-1000:]
