"""The batch lists of tests/test_gpu_handle_batches.py against the dispatch plans, on the CPU: at the largest batch of a
network's list every launch that loops over windows must run at least two passes with a ragged last one - otherwise the GPU
file would compare handles at batches that never leave the first pass of some kernel.

A launch covers `slots` windows per pass: the workgroups along its window axis times the windows a workgroup takes per pass
(csrc/ral_baseline_plan.hip: 1 for a window-at-a-time kernel, DN_ACT_WINDOWS = 4 for k_dn_act / k_dn_act_b, DN_DESC_WINDOWS
= 16 for the descriptor kernels k_dn_fcn_mid / k_dn_fcn_bmid; the U-Net plan reports its windows per pass).  The ACDAE
weight-gradient kernels split the batch into grid-y contiguous runs of ceil(B / grid y) windows instead: their loop is the
run, and it is ragged when the runs do not tile the batch."""
import math

import pytest

from test_baseline_plan_cpu import ACDAE, DANET, passplan
from test_gpu_handle_batches import NETS, PASS_WINDOWS, UNET_WRAP
from test_unet_plan_cpu import query

DESC = ("k_dn_fcn_mid", "k_dn_fcn_bmid")
UNET_BWD_PART_ROWS = 1024        # UNET_PART_ROWS: scratch rows of the fold, one per backward workgroup
# the three kernels around the U-Net's output layer that the stage plan does not list (ral_unet.hip): (workgroups at most,
# units per workgroup and pass, units of a batch) - k_unet_out: float4s, 256 per workgroup; k_unet_gsums: (window, channel) rows,
# a wave each; k_unet_out_loss: windows, a wave each and two windows per wave and pass
UNET_TAIL = {"k_unet_out": (1024, 256, lambda B, leads, L: B * leads * L // 4),
             "k_unet_gsums": (512, 4, lambda B, leads, L: B * leads),
             "k_unet_out_loss": (256, 16, lambda B, leads, L: B)}


def windows_per_workgroup(kernel):
    return 16 if kernel in DESC else 4 if kernel.startswith("k_dn_act") else 1


def baseline_loops(variant, L, B):
    """[(kernel, layer, passes, ragged)] of every launch of a training forward and a backward pass"""
    out = []
    for backward in (0, 1):
        for layer, kernel, gx, gy, threads, lds, extra in passplan(variant, L, B, backward):
            if kernel.startswith("k_acd_dw"):
                run = math.ceil(B / gy)                      # windows [y run, min(B, (y + 1) run)) of split y
                out.append((kernel, layer, run, gy * run != B))
            else:
                slots = gx * windows_per_workgroup(kernel)
                assert gx <= B, (kernel, gx, B)
                out.append((kernel, layer, math.ceil(B / slots), B % slots != 0))
    return out


def unet_loops(leads, L, B, modes=("train", "bwd")):
    out = []
    for mode in modes:
        for si in range(11):
            kernel, grid, wp, threads, lds, fold, fused = query(mode, leads, L, B, si)
            slots = grid * wp
            out.append((kernel, si, math.ceil(B / slots), B % slots != 0))
    return out


def never_wrapped(loops_of, batches):
    """the kernels with a launch that runs one pass only at every batch of the list"""
    best = {}
    for B in batches:
        for kernel, layer, passes, ragged in loops_of(B):
            best[(kernel, layer)] = max(best.get((kernel, layer), 0), passes)
    return sorted({k for (k, _), p in best.items() if p < 2})


@pytest.mark.parametrize("name,variant", [("acdae", ACDAE), ("danet", DANET)])
def test_baseline_lists_wrap_every_loop(name, variant):
    n = NETS[name]
    B = max(n["batches"])
    assert B == n["max_batch"]
    loops = baseline_loops(variant, n["L"], B)
    assert len(loops) == (8 + 16 if name == "acdae" else 38 + 38)      # (DANet: 4 launches per cell and 2 more per DAM, each way)
    bad = [r for r in loops if r[2] < 2 or not r[3]]
    assert not bad, bad
    # the eval forward launches what the training forward launches
    assert [r[1:4] for r in passplan(variant, n["L"], B, 0, training=0)] == [r[1:4] for r in passplan(variant, n["L"], B, 0)]
    # the windows (b) picks lie in the first, a middle and the last pass of every launch of the forward pass
    for layer, kernel, gx, gy, threads, lds, extra in passplan(variant, n["L"], B, 0):
        slots = gx * windows_per_workgroup(kernel)
        seen = {w // slots for w in PASS_WINDOWS[name]}
        assert seen == set(range(math.ceil(B / slots))), (kernel, slots, seen)
        assert {slots - 1, slots, B - 1} <= set(PASS_WINDOWS[name]), (kernel, slots)


def test_danet_descriptor_kernels_wrap_only_beyond_4096_windows():
    """sensitivity: without the batches of DANet's list that lie beyond 256 x 16 windows - the largest, 4100, and 4097 next to it -
    exactly the descriptor kernels are reported as never wrapped; with either of them nothing is"""
    n = NETS["danet"]
    loops_of = lambda B: baseline_loops(DANET, n["L"], B)
    assert never_wrapped(loops_of, n["batches"]) == []
    assert never_wrapped(loops_of, [B for B in n["batches"] if B <= 4096]) == sorted(DESC)
    assert never_wrapped(loops_of, [B for B in n["batches"] if B != max(n["batches"])]) == []      # (4097 wraps them as well: one window)
    assert never_wrapped(loops_of, [B for B in n["batches"] if B <= 1024]) == sorted(
        DESC + ("k_dn_conv<17, false>", "k_dn_conv<3, false>", "k_dn_conv<4, true>", "k_dn_conv<18, true>", "k_dn_dam1", "k_dn_out",
                "k_dn_act<4>", "k_dn_act<1>", "k_dn_act_b<4>", "k_dn_act_b<1>",
                "k_dn_conv_b<17, false>", "k_dn_conv_b<3, false>", "k_dn_conv_b<4, true>", "k_dn_conv_b<18, true>"))


def test_unet_lists_wrap_the_backward_and_the_forward_needs_its_own_batch():
    """the backward stages take 2 windows per pass on 512 workgroups: 1030 windows are a full pass and a ragged one, and more
    rows than the fold has (1024) would be a fault.  The forward stages take up to 4 windows per pass: at 1030 they run ONE
    pass whose last workgroup is ragged (344 x 3 = 1032), and their loop wraps only beyond 2048 windows - which is what
    UNET_WRAP (2050 windows) of the GPU file is for, together with the two-windows-per-wave pass of k_unet_out_loss."""
    n = NETS["unet_fold"]
    B = max(n["batches"])
    loops = unet_loops(n["leads"], n["L"], B)
    bwd = [r for r in loops if "bwd" in r[0]]
    fwd = [r for r in loops if "fwd" in r[0]]
    assert len(bwd) == 11 and len(fwd) == 11
    assert all(p == 2 and ragged for _, _, p, ragged in bwd), bwd
    assert all(p == 1 and ragged for _, _, p, ragged in fwd), fwd
    for si in range(11):
        assert query("bwd", n["leads"], n["L"], B, si)[1] <= min(B, UNET_BWD_PART_ROWS)
        assert query("bwd", n["leads"], n["L"], B, si)[5] == 1 and query("bwd", 2, 48, 6, si)[5] == 0       # fold / atomic path
    # the staged eval forward runs the same loop as the training forward
    assert unet_loops(n["leads"], n["L"], B, ("eval",)) == [(k, si, p, r) for k, si, p, r in fwd]
    for si in range(11):        # (b) picks the first, a middle and the ragged last WORKGROUP, and every place within one
        kernel, grid, wp = query("eval", n["leads"], n["L"], B, si)[:3]
        picked = PASS_WINDOWS["unet_fold"]
        assert {0, grid - 1} < {w // wp for w in picked} and {w % wp for w in picked} == set(range(wp)), kernel
        assert (B - 1) // wp == grid - 1 and B % wp != 0
    Bw = UNET_WRAP["max_batch"]
    for si in range(11):
        kernel, grid, wp = query("eval", UNET_WRAP["leads"], UNET_WRAP["L"], Bw, si)[:3]
        assert {w // (grid * wp) for w in PASS_WINDOWS["unet_wrap"]} == {0, 1}, kernel
    wrapped = unet_loops(UNET_WRAP["leads"], UNET_WRAP["L"], Bw)
    assert all(p >= 2 and ragged for _, _, p, ragged in wrapped), wrapped
    assert never_wrapped(lambda b: unet_loops(n["leads"], n["L"], b), n["batches"]) == sorted({r[0] for r in fwd})
    assert never_wrapped(lambda b: unet_loops(n["leads"], n["L"], b), n["batches"] + (Bw,)) == []
    # the kernels around the output layer: which of the two batches wraps which
    tail = {}
    for k, (cap, per, units) in UNET_TAIL.items():
        for b in (B, Bw):
            u = units(b, n["leads"], n["L"])
            grid = min(math.ceil(u / (per // 2 if k == "k_unet_out_loss" else per)), cap)
            tail[(k, b)] = (math.ceil(u / (grid * per)), u % (grid * per) != 0)
    assert tail[("k_unet_gsums", B)] == (2, True) and tail[("k_unet_gsums", Bw)] == (3, True)
    assert tail[("k_unet_out_loss", B)] == (1, True) and tail[("k_unet_out_loss", Bw)] == (1, True)
    # 2050 windows: stride 2048 - the first two waves take a second window in their pass, which no batch up to 2048 does
    assert min(math.ceil(B / 8), 256) * 8 >= B and min(math.ceil(Bw / 8), 256) * 8 == Bw - 2
    # k_unet_out wraps beyond 1024 x 256 float4s only (tests/test_gpu_unet.py at 2048 x 2 x 512: two full passes)
    assert tail[("k_unet_out", B)][0] == 1 and tail[("k_unet_out", Bw)][0] == 1 and 2048 * 2 * 512 // 4 == 2 * 1024 * 256


def test_small_lists_take_the_paths_they_are_named_after():
    a, s = NETS["unet_atomic"], NETS["unet_staged"]
    assert [query("bwd", a["leads"], a["L"], 6, si)[5] for si in range(11)] == [0] * 11              # no fold: gradient atomics
    assert [query("bwd", s["leads"], s["L"], 4, si)[5] for si in range(11)] == [1] * 11
    assert query("eval", s["leads"], s["L"], 4, 0)[6] == 0 and query("eval", 2, 256, 4, 0)[6] == 1    # stage by stage / one kernel
    assert query("eval", 2, 64, 4, 0)[6] == 0
