"""The baselines' max-pool kernels where several inputs hold the maximum (inputs and premises: tests/tie_util.py,
tests/test_ties_cpu.py).  The reference sends the gradient to the FIRST maximum; only the input gradient can see another
choice (no parameter gradient moves, test_ties_cpu.py), and a batch norm would let one wrong window hide among the others, so
dx is compared per window.

  ACDAE  k_acd_enc_fwd<13>, k_acd_enc_fwd<7>, k_acd_enc_fwd_m<7> record the choice (`acc[1] > acc[0]`), k_acd_enc_bwd routes by it.
  DANet  k_dn_bn_b routes the channel attention's max over L to the first arg-max of a (arg-min where the BatchNorm gain is
         negative), on its fast row path (all cells at L = 256) and its wave-per-row path (the 512-long cell at L = 1024).

The device's convolutions sum a position's taps in an order that does not depend on the position (one fmaf chain per output in
k_acd_enc_fwd and k_dn_conv, one K sweep per MFMA tile in k_acd_enc_fwd_m), so equal inputs give bit-equal outputs and the device
has every tie the network has: every window is held to the bars, none is set aside.  It is torch's CPU convolution that does not
keep that on every host (tie_util.py, `conv1d_by_taps`): with it the fp64 oracle on the MI355X machine's host lost a few flat
pairs and every periodic row to a last bit, chose among them by rounding noise and stood 8e-4 to 1.7e-2 per window away from
the device AND from its own result on another host, while the device stood 1e-6 from that other host's.  The oracles
therefore run on tie_util's position-independent convolutions here (fp64 for the reference, fp32 for e32)."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import ralenet_oracle as O
import tie_util as T
from parity_util import DANET_ZERO, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("L", T.ACDAE_LS)
def test_acdae_first_element_wins_a_tied_pool_pair(L):
    """One train step on the six tie windows against the fp64 oracle: output 1e-5, parameter gradients 1e-4, dx per window 1e-4
    (the fp32 CPU oracle is 5e-7 from fp64 there; a pool whose second element wins costs 1e-1 to 5e-1).
    Observed on an MI355X, L = 64 / 192 / 256: output 4.2e-7 / 3.9e-7 / 4.7e-7, worst parameter gradient 3.9e-7 / 2.1e-7 / 2.5e-7,
    worst window's dx 6.6e-7 / 3.6e-7 / 4.4e-7 (the random window; the all-zero one 2.0e-7 / 2.5e-7 / 2.3e-7)."""
    from ecg_denoise_amd import ACDAE
    p32 = O.init_params(O.acdae_param_shapes(), 1234)
    x, tgt = T.acdae_tie_windows(L)
    ref = T.acdae_oracle_step(p32, x, tgt, torch.float64)
    m = ACDAE(L=L, max_batch=T.ACDAE_B, device=DEV)
    m.load_state_dict(p32)
    m.train()
    y = m(x.to(DEV))
    loss, _, _ = m.loss_and_metrics(y, tgt.to(DEV))
    dx = m.backward(want_dx=True)
    torch.cuda.synchronize()
    ng = m.named_grads()
    ey = rel(y.cpu().numpy(), ref["y"].numpy())
    eg = {k: rel(ng[k].cpu().numpy(), g.numpy()) for k, g in ref["grads"].items()}
    ex = T.per_window(dx.cpu().numpy(), ref["dx"].numpy())
    print(f"[ties] ACDAE L={L}: output {ey:.2e}, worst parameter gradient {max(eg.values()):.2e} ({max(eg, key=eg.get)}), dx per window {ex}")
    assert ey < 1e-5
    assert abs(loss.item() - ref["loss"]) < 1e-5 * abs(ref["loss"])
    bad = {k: e for k, e in eg.items() if not e < 1e-4}
    assert not bad, bad
    assert (ex < 1e-4).all(), ex


def _danet_step(st64, x, tgt):
    """the handle's training forward and backward on (x, tgt) -> (its errors against the fp64 oracle, e32 per tensor)"""
    from ecg_denoise_amd import DANet
    st32 = OrderedDict((k, v.clone().float() if v.dtype.is_floating_point else v.clone()) for k, v in st64.items())
    ref, r32 = T.danet_oracle_step(st64, x, tgt), T.danet_oracle_step(st32, x, tgt)
    B, _, L = x.shape
    m = DANet(L=L, max_batch=B, train=True, device=DEV)
    m.load_state_dict(st32)
    m.train()
    y = m(x.to(DEV))
    loss, _, _ = m.loss_and_metrics(y, tgt.to(DEV))
    dx = m.backward(want_dx=True)
    torch.cuda.synchronize()
    err = dict(y=rel(y.cpu().numpy(), ref["y"].numpy()), loss=abs(loss.item() - ref["loss"]) / ref["loss"],
               dx=T.per_window(dx.cpu().numpy(), ref["dx"].numpy()), grads={}, zero={})
    e32 = {}
    for k, v in m.named_grads().items():
        if k.endswith(DANET_ZERO):
            err["zero"][k] = v.abs().max().item()
        else:
            err["grads"][k] = rel(v.cpu().numpy(), ref["grads"][k].numpy())
            e32[k] = rel(r32["grads"][k].numpy(), ref["grads"][k].numpy())
    assert set(err["grads"]) | set(err["zero"]) == set(ref["grads"])
    return err, e32, T.per_window(r32["dx"].numpy(), ref["dx"].numpy())


def _report(what, err, e32, e32x):
    worst = max(err["grads"], key=lambda k: err["grads"][k] / max(1e-4, 4 * e32[k]))
    print(f"[ties] DANet {what}: output {err['y']:.2e}, loss {err['loss']:.2e}, dx per window {err['dx']} (fp32 oracle {e32x.max():.1e}), "
          f"worst tensor {worst}: e32 {e32[worst]:.2e}, bar {max(1e-4, 4 * e32[worst]):.2e}, observed {err['grads'][worst]:.2e}; "
          f"largest e32 {max(e32.values()):.2e} ({max(e32, key=e32.get)})")


@pytest.mark.parametrize("case", T.DANET_CASES, ids=lambda c: "%d-%d-%d" % c)
def test_danet_first_maximum_takes_the_pooled_gradient(case):
    """Training forward and backward on the periodic batch with the negated-gain state: output and loss 1e-5, dx per window 1e-4
    (the fp32 CPU oracle is at most 2e-6 from fp64 there; the even split over tied maxima costs 5e-3 at least on every periodic window).
    Parameter gradients against max(1e-4, 4 x e32), e32 being the fp32 CPU oracle's own deviation from fp64 for that tensor,
    computed here: a small cancelling gradient is not known better than that in fp32.
    Observed on an MI355X (worst tensor by error over bar: e32 / bar / observed):
      (256, 32, 8):  dec.DecoderList.3.activate.fcn.1.bias 2.9e-6 / 1.0e-4 / 6.6e-6; largest e32 7.0e-6; output 4.2e-7, loss 6.2e-8,
                     dx per window at most 1.0e-6 (periodic windows 3.4e-7 to 6.9e-7; fp32 oracle 7.2e-7)
      (1024, 64, 8): dec.DecoderList.2.activate.fcn.4.weight 1.1e-5 / 1.0e-4 / 1.6e-5; largest e32 2.1e-5; output 7.4e-7, loss 1.9e-8,
                     dx per window at most 3.4e-6 (periodic windows 4.4e-7 to 9.8e-7; fp32 oracle 2.1e-6)
    No e32 reaches 2.5e-5, so every bar is 1e-4 here."""
    x, tgt = T.danet_tie_batch(*case)
    err, e32, e32x = _danet_step(T.danet_negated_state(torch.float64), x, tgt)
    _report(case, err, e32, e32x)
    assert err["y"] < 1e-5 and err["loss"] < 1e-5
    assert (err["dx"] < 1e-4).all(), err["dx"]
    bad = {k: (e, e32[k]) for k, e in err["grads"].items() if not e < max(1e-4, 4 * e32[k])}
    assert not bad, bad
    assert max(err["zero"].values()) < 1e-5, err["zero"]


def test_danet_negative_gains_on_windows_without_ties():
    """The same state on plain randn windows (8, 2, 256): k_dn_bn_b's `up == false` side (the maximum of x = BN(a) at the minimum
    of a) with nothing else unusual, at the bars of test_gpu_danet.py: forward 1e-5, every gradient 1e-4.
    Observed on an MI355X: output 1.6e-6, loss 1.0e-8, dx per window at most 1.4e-5, worst parameter gradient 6.6e-5
    (dec.DecoderList.1.dam.convsa.weight, where the fp32 CPU oracle itself is 3.7e-5 from fp64)."""
    x, tgt = T.danet_random_batch()
    err, e32, e32x = _danet_step(T.danet_negated_state(torch.float64), x, tgt)
    _report("randn (8, 2, 256)", err, e32, e32x)
    assert err["y"] < 1e-5 and err["loss"] < 1e-5
    assert (err["dx"] < 1e-4).all(), err["dx"]
    bad = {k: e for k, e in err["grads"].items() if not e < 1e-4}
    assert not bad, bad
    assert max(err["zero"].values()) < 1e-5, err["zero"]
