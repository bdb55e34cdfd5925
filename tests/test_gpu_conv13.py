"""The two kernels of the 12-lead adapter as operators: ral_conv13_forward / ral_conv13_backward (Conv1d(cin, cout, 13, padding 6)
[+ LeakyReLU(0.01)], channel-major (B, C, L)) on torch tensors against F.conv1d + F.leaky_relu in fp64 with autograd.

Channel pairs: the model's four - (12, 6), (6, 2), (2, 6) with LeakyReLU, (6, 12) without - and (1, 1), (12, 6) without LeakyReLU
and (3, 5) beside them.  Shapes (B, L): (2, 5) and (3, 100) for every pair (a row shorter than the halo; L not a multiple of 4);
for the model's pairs also (1, 1), (3, 13), (513, 16) and (1025, 16) - k_conv13_bwd has 512 workgroups: workgroup 0 takes two /
three windows, the others one / two, with the weight-gradient accumulators carried over the restaged LDS - and, forward only,
(2049, 16) and (4097, 4): k_conv13_fwd has 2048 workgroups.  (12, 6) with LeakyReLU alone runs (2, 2048), the largest LDS request
of the model (152 080 of 163 840 bytes in the backward kernel).

Every backward case checks the += contract of gw and gb (pre-filled with nonzero values: result = prefill + gradient), and
the dx = NULL branch in a second call; one case has a window of zeros under a zero bias, y == 0 exactly, where the gradient
follows torch's convention (slope 0.01 at 0).  The backward kernel reads the oracle's y rounded to fp32, so that both sides
take the same branch of the LeakyReLU everywhere.

Bars: those of tests/test_gpu_parity.py, 1e-5 forward and 1e-4 gradients, applied to the relative L2 error and to
max|got - ref| / max|ref| (one wrong edge sample would vanish in the L2 norm of a 2048-sample row).

Observed worst errors on an MI355X (relative L2 / elementwise):
  y                        2.6e-7 / 6.4e-7      (worst: 12 -> 6 at (3, 13) / (513, 16))
  dx                       2.2e-7 / 5.7e-7      (6 -> 12 at (3, 100) / (513, 16))
  gw, gb into zeros        8.4e-7 / 1.4e-6      (gb 6 -> 2 at (513, 16) / gw 12 -> 6 at (2, 2048))
  gw, gb on a prefill      2.1e-6 / 5.0e-6      (gw 12 -> 6 at (513, 16) / 6 -> 12 at (513, 16): the prefill's own fp32 rounding)
  dx of the zero window    1.7e-7 / 3.0e-7      (the kink case, on the window's own scale)"""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from ecg_denoise_amd import _lib
from parity_bars import FWD_TOL, GRAD_TOL
from parity_util import rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

MODEL_PAIRS = [(12, 6, 1), (6, 2, 1), (2, 6, 1), (6, 12, 0)]
OTHER_PAIRS = [(1, 1, 0), (12, 6, 0), (3, 5, 1)]
BWD_CASES = ([p + s for p in MODEL_PAIRS + OTHER_PAIRS for s in ((2, 5), (3, 100))]
             + [p + s for p in MODEL_PAIRS for s in ((1, 1), (3, 13), (513, 16), (1025, 16))]
             + [(12, 6, 1, 2, 2048)])
FWD_CASES = [p + s for p in MODEL_PAIRS for s in ((2049, 16), (4097, 4))]


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _elem(got, ref):
    """max |got - ref| / max |ref|"""
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


@functools.lru_cache(maxsize=None)
def _case(cin, cout, lrelu, B, L, kink=False, backward=True):
    """seeded inputs (fp32) and the fp64 oracle of one case, computed once: x, w, b, dy, y, dx, gw, gb"""
    g = torch.Generator().manual_seed(1000 * cin + 100 * cout + 10 * lrelu + B + L)
    x = torch.randn(B, cin, L, generator=g)
    bound = 1.0 / (cin * 13) ** 0.5
    w = (torch.rand(cout, cin, 13, generator=g) * 2 - 1) * bound
    b = (torch.rand(cout, generator=g) * 2 - 1) * bound
    dy = torch.randn(B, cout, L, generator=g)
    if kink:
        x[B // 2] = 0.0
        b.zero_()
    xo, wo, bo = (t.double().requires_grad_(True) for t in (x, w, b))
    y = F.conv1d(xo, wo, bo, padding=6)
    if lrelu:
        y = F.leaky_relu(y, 0.01)
    out = dict(x=x, w=w, b=b, dy=dy, y=y.detach())
    if backward:
        out["dx"], out["gw"], out["gb"] = torch.autograd.grad(y, [xo, wo, bo], dy.double())
    return out


def _forward(c, cin, cout, lrelu, B, L):
    x, w, b = (c[k].to(DEV) for k in ("x", "w", "b"))
    y = torch.full((B, cout, L), float("nan"), device=DEV)
    _lib.check(_lib.lib().ral_conv13_forward(_vp(x), _vp(w), _vp(b), _vp(y), B, cin, cout, L, lrelu, _stream()))
    torch.cuda.synchronize()
    return y


def _backward(c, cin, cout, lrelu, B, L, want_dx, prefill):
    """-> (dx or None, gw - prefill, gb - prefill) with the subtraction in fp64"""
    x, w, dy = (c[k].to(DEV) for k in ("x", "w", "dy"))
    y = c["y"].float().to(DEV)
    g = torch.Generator().manual_seed(7)
    # the prefill has the gradient's own size: the fp32 rounding of prefill + gradient stays at the gradient's rounding level
    pw = torch.randn(cout, cin, 13, generator=g) * c["gw"].abs().max().float() if prefill else torch.zeros(cout, cin, 13)
    pb = torch.randn(cout, generator=g) * c["gb"].abs().max().float() if prefill else torch.zeros(cout)
    gw, gb = pw.to(DEV), pb.to(DEV)
    dx = torch.full((B, cin, L), float("nan"), device=DEV) if want_dx else None
    _lib.check(_lib.lib().ral_conv13_backward(_vp(x), _vp(y), _vp(dy), _vp(w), _vp(gw), _vp(gb), _vp(dx), B, cin, cout, L, lrelu, _stream()))
    torch.cuda.synchronize()
    if prefill:
        assert pw.abs().min().item() > 0 and pb.abs().min().item() > 0
    return dx, gw.double().cpu() - pw.double(), gb.double().cpu() - pb.double()


def _check(errs, what):
    print(f"\nobserved {what}: " + ", ".join(f"{k} {l2:.2e} / {el:.2e}" for k, (l2, el, _) in errs.items()))
    bad = {k: (l2, el) for k, (l2, el, tol) in errs.items() if not (l2 <= tol and el <= tol)}
    assert not bad, bad


def _both(got, ref, tol):
    return rel(got.cpu().numpy(), ref.numpy()), _elem(got, ref), tol


def _run_backward_case(cin, cout, lrelu, B, L, kink=False):
    c = _case(cin, cout, lrelu, B, L, kink)
    errs = {"y": _both(_forward(c, cin, cout, lrelu, B, L), c["y"], FWD_TOL)}
    dx, gw, gb = _backward(c, cin, cout, lrelu, B, L, True, True)
    errs["dx"] = _both(dx, c["dx"], GRAD_TOL)
    errs["gw+="] = _both(gw, c["gw"], GRAD_TOL)
    errs["gb+="] = _both(gb, c["gb"], GRAD_TOL)
    _, gw0, gb0 = _backward(c, cin, cout, lrelu, B, L, False, False)
    errs["gw(dx=NULL)"] = _both(gw0, c["gw"], GRAD_TOL)
    errs["gb(dx=NULL)"] = _both(gb0, c["gb"], GRAD_TOL)
    return c, dx, errs


@pytest.mark.parametrize("cin,cout,lrelu,B,L", BWD_CASES)
def test_conv13_forward_and_backward_match_oracle(cin, cout, lrelu, B, L):
    _, _, errs = _run_backward_case(cin, cout, lrelu, B, L)
    _check(errs, f"{cin}->{cout} lrelu={lrelu} B={B} L={L}")


@pytest.mark.parametrize("cin,cout,lrelu,B,L", FWD_CASES)
def test_conv13_forward_beyond_its_grid_matches_oracle(cin, cout, lrelu, B, L):
    c = _case(cin, cout, lrelu, B, L, backward=False)
    _check({"y": _both(_forward(c, cin, cout, lrelu, B, L), c["y"], FWD_TOL)}, f"{cin}->{cout} lrelu={lrelu} B={B} L={L}")


def test_conv13_gradient_at_the_leaky_relu_kink():
    """a window of zeros under a zero bias: y == 0 exactly in that window, where torch's LeakyReLU has slope 0.01"""
    cin, cout, B, L = 12, 6, 3, 100
    c, dx, errs = _run_backward_case(cin, cout, 1, B, L, kink=True)
    z = B // 2
    assert c["y"][z].abs().max().item() == 0.0 and c["y"].abs().min().item() == 0.0
    errs["dx[zero window]"] = _both(dx[z], c["dx"][z], GRAD_TOL)       # (on its own scale: 1 / 100 of the other windows')
    assert c["dx"][z].abs().max().item() > 0
    _check(errs, f"kink {cin}->{cout} B={B} L={L}")
