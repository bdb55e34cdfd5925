"""Inputs on which a max-pool has to choose between equal maxima, for the two baselines that have one (tests/test_ties_cpu.py
checks the premises on the CPU oracle, tests/test_gpu_ties.py runs the kernels on them; oracle/gen_golden_danet.py makes the
reference fixture g3_danet_ties_L256.npz from the same builders).

ECG gives such windows: a lead-off or rail-clipped stretch is exactly flat, a patient simulator repeats one beat bit for bit.
  ACDAE  MaxPool1d(2) after each encoder convolution: a flat stretch makes both inputs of a pair equal.  The reference
         (F.max_pool1d) sends the gradient to the FIRST of them.
  DANet  the DAM's AdaptiveMaxPool1d(1) over L: a window that repeats one beat attains its maximum once per period, and the
         reference sends the gradient to the first of them."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

import danet_oracle as D
import ralenet_oracle as O
from parity_bars import standing_in

ACDAE_LS = (64, 192, 256)            # the ACDAE lengths of the GPU test (test_ties_cpu.py: the kernels they launch between them)
ACDAE_B = 6
DANET_CASES = ((256, 32, 8), (1024, 64, 8))      # (L, period, B)
DANET_STATE_SEED = 99
# channels of dec.DecoderList.{0,1,2}.bn.weight whose gain is negated: there k_dn_bn_b finds the maximum of x = BN(a) at the
# MINIMUM of a.  Chosen with BEAT_SEED so that each DAM cell of both cases has tied rows on both kinds of channel
# (test_ties_cpu.py holds the counts)
NEGATED = {0: (0, 3, 4, 10, 11, 15), 1: (3, 5, 6, 7), 2: (0, 3)}
BEAT_SEED = 2


# ---------------------------------------------------------------------------------------------------------------- ACDAE
def acdae_tie_windows(L, seed=2023):
    """(x, target), both (6, 2, L) fp32.  Windows: 0 the middle half of both leads is 0 (lead-off); 1 clamp(-0.5, 0.5) (rails);
    2 lead 0 all 0; 3 samples rounded to eighths (a coarse ADC); 4 both leads all 0 - a partial stretch is too short to
    reach encoder 3 at a short L, this one ties at every level; 5 randn, no tie.  The target of a window is its neighbour
    (the batch rolled by one), so that no window's error is flat."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(ACDAE_B, 2, L, generator=g)
    x[0, :, L // 4:3 * L // 4] = 0.0
    x[1] = x[1].clamp(-0.5, 0.5)
    x[2, 0] = 0.0
    x[3] = torch.round(x[3] * 8) / 8
    x[4] = 0.0
    return x, torch.roll(x, 1, 0)


def second_wins_max_pool1d(x, k):
    """MaxPool1d(2) whose SECOND element wins a tie: F.max_pool1d on the mirrored signal"""
    assert k == 2 and x.shape[-1] % 2 == 0
    return F.max_pool1d(x.flip(-1), 2).flip(-1)


# ---- convolutions whose rounding does not depend on the position.  A tie needs two outputs that see equal inputs to be equal
# bit for bit.  The library convolutions of torch on the CPU do not promise that and, measured, do not keep it on every machine:
# on one host flat and periodic inputs gave bit-equal outputs at every thread count, on another (other vector units, same
# torch) 11 of 128 flat pairs of ACDAE's encoder 2 at L = 64 and every periodic DAM row of DANet came out a last bit apart,
# in fp64 too, with one thread and without oneDNN as well - the oracle then has no tie where the network has one, and picks
# by rounding noise.  So the tie tests run the oracles on these: one elementwise multiply and one elementwise add per (input
# channel, tap), the same chain of IEEE operations at every position.  They agree with F.conv1d / F.conv_transpose1d to
# 1e-15 (test_ties_cpu.py), which is all the oracle's other users ask of a convolution.
def conv1d_by_taps(x, w, b=None, stride=1, padding=0):
    xp = F.pad(x, (padding, padding))
    co, ci_n, K = w.shape
    lout = (xp.shape[-1] - K) // stride + 1
    out = None
    for k in range(K):
        xs = xp[:, :, k:k + stride * (lout - 1) + 1:stride]
        for ci in range(ci_n):
            t = w[:, ci, k].view(1, co, 1) * xs[:, ci:ci + 1, :]
            out = t if out is None else out + t
    return out if b is None else out + b.view(1, -1, 1)


def conv_transpose1d_by_taps(x, w, b=None, stride=1, padding=0):
    """the input with stride - 1 zeros between its samples, convolved with the mirrored kernel (a zero term changes no sum)"""
    B, ci_n, lin = x.shape
    z = x
    if stride > 1:
        z = x.new_zeros(B, ci_n, (lin - 1) * stride + 1)
        z[:, :, ::stride] = x
    return conv1d_by_taps(z, w.flip(2).transpose(0, 1), b, 1, w.shape[2] - 1 - padding)


def oracle_functional(mod, **attrs):
    """oracle module `mod` (ralenet_oracle, danet_oracle) on the convolutions by taps, with `attrs` as parity_bars.standing_in's"""
    taps = dict(conv1d=conv1d_by_taps, conv_transpose1d=conv_transpose1d_by_taps)
    return standing_in(mod, F=dict(taps, **attrs.pop("F", {})), **attrs)


def acdae_oracle_step(p32, x, tgt, dtype, pool=None):
    """one forward and backward of the ACDAE oracle in `dtype`, `pool(x, 2)` in place of F.max_pool1d -> dict(y, loss,
    grads {name: tensor}, dx, pooled [the four encoder convolutions' outputs, the inputs of the pools])"""
    p = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in p32.items())
    xd = x.detach().to(dtype).clone().requires_grad_(True)
    seen = []

    def rec(t, k):
        seen.append(t.detach())
        return (pool or F.max_pool1d)(t, k)

    with oracle_functional(O, F=dict(max_pool1d=rec)):
        y = O.acdae_forward(p, xd)
    loss = O.mse(y, tgt.to(dtype))
    gr = torch.autograd.grad(loss, list(p.values()) + [xd])
    return dict(y=y.detach(), loss=loss.item(), grads=OrderedDict(zip(p.keys(), gr[:-1])), dx=gr[-1], pooled=seen)


def pool_pairs(t, near=1e-9):
    """(tied, near) boolean arrays over the pairs of a MaxPool1d(2) input: exactly equal; unequal but within `near` relative"""
    a, b = t[..., 0::2].numpy(), t[..., 1::2].numpy()
    tied = a == b
    return tied, ~tied & (np.abs(a - b) <= near * np.maximum(np.abs(a), np.abs(b)))


# ---------------------------------------------------------------------------------------------------------------- DANet
def danet_tie_batch(L, period, B, seed=BEAT_SEED):
    """(x, target), both (B, 2, L) fp32: every even window is one random two-lead beat of `period` samples repeated L / period
    times, every odd window and every target is randn"""
    assert L % period == 0
    g = torch.Generator().manual_seed(seed * 1000 + L)
    x = torch.randn(B, 2, L, generator=g); tgt = torch.randn(B, 2, L, generator=g)
    for b in range(0, B, 2):
        x[b] = torch.randn(2, period, generator=g).repeat(1, L // period)
    return x, tgt


def danet_random_batch(L=256, B=8, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 2, L, generator=g), torch.randn(B, 2, L, generator=g)


def danet_negated_state(dtype=torch.float64):
    """init_state(99) with the gains of NEGATED's channels of the three DAM cells' BatchNorms negated (init_state draws every
    gain as 1 + 0.1 N(0, 1): without this no gain is negative)"""
    st = D.init_state(DANET_STATE_SEED, dtype=dtype)
    for i, chans in NEGATED.items():
        w = st[f"dec.DecoderList.{i}.bn.weight"]
        assert (w > 0).all()
        w[list(chans)] *= -1
    return st


def danet_oracle_step(st, x, tgt):
    """one training forward and backward of the DANet oracle in the dtype of `st` (a fresh copy of it) -> dict(y, loss, grads,
    dx, dam [the inputs of the three DAM cells, (B, C, lout)], state [after the step])"""
    st = OrderedDict((k, v.clone()) for k, v in st.items())
    for k in st:
        if ".dam.fcn2." in k:
            st[k] = st[k.replace(".dam.fcn2.", ".dam.fcn1.")]
    dtype = st["enc.EncoderList.cell0.conv.weight"].dtype
    params = OrderedDict((k, v.requires_grad_(True)) for k, v in st.items() if D.is_param(k) and ".dam.fcn2." not in k)
    xd = x.detach().to(dtype).clone().requires_grad_(True)
    seen = []
    keep = D._dam

    def rec(t, *a):
        seen.append(t.detach())
        return keep(t, *a)

    with oracle_functional(D, _dam=rec):
        y = D.danet_forward(st, xd, training=True)
    loss = F.mse_loss(y, tgt.to(dtype))
    loss.backward()
    return dict(y=y.detach(), loss=loss.item(), grads=OrderedDict((k, v.grad) for k, v in params.items()), dx=xd.grad, dam=seen, state=st)


def first_max(t):
    """per (window, channel) row of a DAM input: (index of the first maximum over L, how many positions hold it)"""
    a = t.numpy()
    hit = a == a.max(-1, keepdims=True)
    return hit.argmax(-1), hit.sum(-1)          # (numpy's argmax returns the first occurrence)


def per_window(a, b):
    """relative L2 deviation of a from b per window -> (B,); a window whose reference is all zero counts absolutely"""
    a = np.asarray(a, dtype=np.float64).reshape(len(a), -1); b = np.asarray(b, dtype=np.float64).reshape(len(b), -1)
    return np.linalg.norm(a - b, axis=1) / np.maximum(np.linalg.norm(b, axis=1), 1e-30)


# k_dn_bn_b's choice between its two forms (ral_danet.hip, `rowfast`): a channel row is q4 = lout / 4 consecutive lanes of one wave
def bn_b_rowfast(c, lout):
    q4, n4w = lout >> 2, (c * lout) >> 2
    return lout % 4 == 0 and q4 <= 64 and q4 & (q4 - 1) == 0 and n4w % 64 == 0
