"""The premises of tests/test_gpu_ties.py, on the CPU oracle alone: the inputs of tests/tie_util.py really make the two baselines'
max-pools choose between equal maxima, fp32 and fp64 arithmetic agree on where, the choice is visible in the input gradient,
and the chosen shapes launch the kernels (and, inside k_dn_bn_b, take the code paths) that carry a tie rule.  The oracles run
on tie_util's convolutions by taps: with torch's own the counts below hold on some hosts and not on others."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest
import torch

import ralenet_oracle as O
import tie_util as T
from ecg_denoise_amd import _lib
from parity_util import rel
from test_baseline_plan_cpu import ACDAE, DANET, passplan


def _acdae_params():
    return O.init_params(O.acdae_param_shapes(), 1234)


@pytest.fixture(scope="module")
def acdae_steps():
    """{L: (fp64 step, fp32 step)} of the ACDAE oracle on the tie windows"""
    p32 = _acdae_params()
    out = {}
    for L in T.ACDAE_LS:
        x, tgt = T.acdae_tie_windows(L)
        out[L] = (T.acdae_oracle_step(p32, x, tgt, torch.float64), T.acdae_oracle_step(p32, x, tgt, torch.float32))
    return out


def test_convolutions_by_taps_are_the_library_ones_and_do_not_depend_on_the_position():
    """every (stride, kernel, padding, transposed) of the two networks: equal to torch's convolution to 1e-13 in fp64, gradients
    included, and - what torch's does not promise - a periodic input gives a bit-periodic output away from the padding, in fp64
    and in fp32"""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(4)
    for cin, cout, k, pad, stride, tr in [(2, 4, 17, 8, 2, 0), (8, 16, 3, 1, 2, 0), (32, 16, 4, 1, 2, 1), (8, 4, 18, 8, 2, 1),       # DANet
                                          (2, 16, 13, 6, 1, 0), (16, 32, 7, 3, 1, 0), (32, 16, 7, 3, 1, 1)]:                        # ACDAE
        beat = torch.randn(2, cin, 16, generator=g, dtype=torch.float64)
        w = torch.randn(*((cin, cout, k) if tr else (cout, cin, k)), generator=g, dtype=torch.float64)
        b = torch.randn(cout, generator=g, dtype=torch.float64)
        mine, lib = (T.conv_transpose1d_by_taps, F.conv_transpose1d) if tr else (T.conv1d_by_taps, F.conv1d)
        for dtype in (torch.float64, torch.float32):
            x = beat.repeat(1, 1, 6).to(dtype).requires_grad_(True)
            wd = w.to(dtype).requires_grad_(True)
            y = mine(x, wd, b.to(dtype), stride, pad)
            if dtype == torch.float64:
                yl = lib(x, wd, b, stride=stride, padding=pad)
                assert y.shape == yl.shape and rel(y.detach().numpy(), yl.detach().numpy()) < 1e-13
                dy = torch.randn(y.shape, generator=g, dtype=dtype)
                for a, c in zip(torch.autograd.grad(y, [x, wd], dy, retain_graph=True), torch.autograd.grad(yl, [x, wd], dy)):
                    assert rel(a.numpy(), c.numpy()) < 1e-13
            per = 16 * y.shape[-1] // x.shape[-1]             # the output's period
            inner = y.detach()[..., 2 * per:-2 * per]
            assert torch.equal(inner[..., :-per], inner[..., per:]), (cin, cout, k, tr, dtype)


def flat_pairs_of_the_zero_window(L):
    """pool pairs per encoder level that the all-zero window ties by construction.  Encoder 0 turns zeros (zero padding included)
    into its bias at every position.  From then on the input is a non-zero constant and the zero padding of a 'same' convolution
    shows in the 3 outermost outputs of each side; a pair ties when both of its positions are clear of that, and clears the
    pooled position.  The clear stretch loses 3 samples a side per level while the length halves: at L = 64 encoder 3 sees 8
    samples, positions 3 and 4 alone are clear, and no output of a 7-tap convolution is - NO input ties there except by
    coincidence, so L = 64 ties at levels 0 to 2 only (encoder 3's tie rule, direct and MFMA form, runs at L = 192 and 256)."""
    clear = np.ones(L, bool)
    out = []
    for lvl in range(4):
        if lvl:
            pad = np.concatenate([np.zeros(3, bool), clear, np.zeros(3, bool)])
            clear = np.array([pad[p:p + 7].all() for p in range(len(clear))])
        clear = clear[0::2] & clear[1::2]
        out.append(int(clear.sum()))
    return out


@pytest.mark.parametrize("L", T.ACDAE_LS)
def test_acdae_windows_tie_at_every_encoder_level_in_fp32_as_in_fp64(acdae_steps, L):
    """Exactly tied MaxPool1d(2) pairs of the four encoder levels over the 6 windows:
        L = 64: 672 / 448 / 128 / 0      L = 192: 2208 / 1984 / 1536 / 768      L = 256: 2976 / 2752 / 2304 / 1536
    (the 0: flat_pairs_of_the_zero_window), at least what the all-zero window ties by construction, the same pairs in the fp32
    oracle, and no other pair within 1e-9 relative of a tie in fp64 - a near-tie is where fp32 arithmetic (the oracle's or the
    device's) could decide differently from fp64 without being wrong, so the cap is 0.  fp32 against fp64: dx per window 5e-7
    at worst."""
    r64, r32 = acdae_steps[L]
    counts = []
    flat = flat_pairs_of_the_zero_window(L)
    assert all(n >= 1 for n in flat) if L > 64 else (all(n >= 1 for n in flat[:3]) and flat[3] == 0)
    for lvl in range(4):
        t64, n64 = T.pool_pairs(r64["pooled"][lvl])
        t32, n32 = T.pool_pairs(r32["pooled"][lvl])
        counts.append(int(t64.sum()))
        assert t64[4].sum() >= O.ACDAE_CH[lvl + 1] * flat[lvl], (L, lvl)
        assert t64.sum() >= 1 or (L, lvl) == (64, 3), (L, lvl)
        assert (t64 == t32).all(), (L, lvl, int((t64 != t32).sum()))
        assert n64.sum() == 0, (L, lvl, int(n64.sum()))
    e = T.per_window(r32["dx"].numpy(), r64["dx"].numpy())
    print(f"[ties] ACDAE L={L}: tied pairs per level {counts}; fp32 against fp64 dx per window {e.max():.1e}")
    assert e.max() < 1e-5                       # (the bar of the GPU test is 1e-4)


@pytest.mark.parametrize("L", T.ACDAE_LS)
def test_acdae_input_gradient_sees_a_pool_whose_second_element_wins(acdae_steps, L):
    """F.max_pool1d swapped for its mirror: the same forward, and an input gradient that moves by 0.53 / 0.11 / 0.14 relative L2 at
    L = 64 / 192 / 256 - a thousand times the bar of the GPU test.  No parameter gradient moves (at most 2e-16: in a flat
    stretch both elements of a pair see the same input), so only dx can tell."""
    r64, _ = acdae_steps[L]
    x, tgt = T.acdae_tie_windows(L)
    m = T.acdae_oracle_step(_acdae_params(), x, tgt, torch.float64, pool=T.second_wins_max_pool1d)
    assert torch.equal(m["y"], r64["y"])
    d = rel(m["dx"].numpy(), r64["dx"].numpy())
    dp = max(rel(m["grads"][k].numpy(), g.numpy()) for k, g in r64["grads"].items())
    print(f"[ties] ACDAE L={L}: second-wins pool moves dx by {d:.2f}, the parameter gradients by {dp:.1e}")
    assert d > 1e-2
    # per window: the flat windows move, the random one does not
    e = T.per_window(m["dx"].numpy(), r64["dx"].numpy())
    assert e[4] > 1e-2 and e[5] == 0.0, e


@pytest.fixture(scope="module")
def danet_steps():
    st64 = T.danet_negated_state(torch.float64)
    st32 = OrderedDict((k, v.float() if v.dtype.is_floating_point else v.clone()) for k, v in st64.items())
    out = {}
    for case in T.DANET_CASES:
        x, tgt = T.danet_tie_batch(*case)
        out[case] = (T.danet_oracle_step(st64, x, tgt), T.danet_oracle_step(st32, x, tgt))
    return out


@pytest.mark.parametrize("case", T.DANET_CASES, ids=lambda c: "%d-%d-%d" % c)
def test_danet_periodic_windows_tie_in_every_dam_cell_on_both_kinds_of_channel(danet_steps, case):
    """(window, channel) rows of the three DAM cells' inputs whose maximum over L is attained more than once, on channels with a
    positive / a negated BatchNorm gain (NEGATED and BEAT_SEED of tie_util.py were chosen for these):
        (256, 32, 8):   9 / 7,  4 / 6,  3 / 1        (1024, 64, 8):  20 / 14,  8 / 10,  5 / 2
    All of them lie in the periodic (even) windows.  The fp32 oracle has the same first index and the same multiplicity in every
    row of every cell, so a device that computes in fp32 is asked a question with one answer."""
    r64, r32 = danet_steps[case]
    assert len(r64["dam"]) == 3
    got = []
    for i in range(3):
        t = r64["dam"][i]
        i64, n64 = T.first_max(t); i32, n32 = T.first_max(r32["dam"][i])
        neg = np.zeros(t.shape[1], bool); neg[list(T.NEGATED[i])] = True
        tied = n64 > 1
        got.append((int(tied[:, ~neg].sum()), int(tied[:, neg].sum())))
        assert got[-1][0] >= 2 and got[-1][1] >= 1, (case, i, got)
        assert not tied[1::2].any()
        assert (i64 == i32).all() and (n64 == n32).all(), (case, i)
    e = T.per_window(r32["dx"].numpy(), r64["dx"].numpy())
    print(f"[ties] DANet {case}: tied rows per cell (positive gain, negated gain) {got}; fp32 against fp64 dx per window {e.max():.1e}")
    assert e.max() < 2.5e-5                     # (the bar of the GPU test is 1e-4)


def test_the_negated_state_has_both_signs_in_each_dam_cell_and_nowhere_else():
    st, base = T.danet_negated_state(), T.D.init_state(T.DANET_STATE_SEED, dtype=torch.float64)
    for k in st:
        if k.endswith("bn.weight") and k.startswith("dec.DecoderList.") and int(k.split(".")[2]) < 3:
            i = int(k.split(".")[2])
            assert sorted(np.flatnonzero(st[k].numpy() < 0)) == sorted(T.NEGATED[i]) and 0 < len(T.NEGATED[i]) < st[k].numel()
            assert torch.equal(st[k].abs(), base[k])
        elif st[k].dtype.is_floating_point:
            assert torch.equal(st[k], base[k]), k


def test_the_chosen_shapes_reach_every_kernel_and_path_with_a_tie_rule():
    """ACDAE: the three lengths launch both direct encoder forwards, the MFMA one and both encoder backwards (encoder 3 is direct
    only where L is no multiple of 128).  DANet: from the layer table's Geo (c, lout = L >> out_shift, dam), L = 256 puts all
    three DAM cells on k_dn_bn_b's fast row path and L = 1024 puts the 512-long cell on its wave-per-row path."""
    want = {"k_acd_enc_fwd<13>", "k_acd_enc_fwd<7>", "k_acd_enc_fwd_m<7>", "k_acd_enc_bwd<13>", "k_acd_enc_bwd<7>"}
    per_L = {L: {e[1] for b in (0, 1) for e in passplan(ACDAE, L, T.ACDAE_B, b)} for L in T.ACDAE_LS}
    assert want <= set().union(*per_L.values())
    assert "k_acd_enc_fwd<7>" in per_L[64] and "k_acd_enc_fwd<7>" in per_L[192] and "k_acd_enc_fwd<7>" not in per_L[256]
    lib = _lib.lib()
    row = (C.c_int32 * 9)()
    paths = {}
    for L, _, B in T.DANET_CASES:
        assert {"k_dn_bn_b", "k_dn_dam_b", "k_dn_dam1"} <= {e[1] for b in (0, 1) for e in passplan(DANET, L, B, b)}
        for r in range(8):
            assert lib.ral_baseline_layer_geom(DANET, 2, r, row, 9) == 0, lib.ral_last_error()
            cin, c, k, p, tr, ish, osh, in1, dam = tuple(row)
            if dam:
                paths[(L, L >> osh)] = T.bn_b_rowfast(c, L >> osh)
    assert paths == {(256, 32): True, (256, 64): True, (256, 128): True, (1024, 128): True, (1024, 256): True, (1024, 512): False}
