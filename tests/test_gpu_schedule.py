"""The host code that strings the RA-LENet kernels into a step (csrc/ral_ralenet.hip): micro-batch lanes 1 .. 4, weight-gradient
side streams on and off, 2 / 6 / 8 sets of backward temporaries, one handle driven with changing batches, the weight planes
an eval-mode model keeps between forwards, and the profile hooks (`pytest -m gpu`).

Every model is the "full" variant at L = 256 (the smallest length that runs unpadded on the default fp16-pair kernels) with
R-wave tables of 0.3 * randn (zero tables would hide the bias path); 64 windows per lane is the smallest batch the
library splits.  The schedule a step ran is read off the library's event timeline by tests/schedule_util.py; the `[schedule]`
lines (run with -s) give the lanes found, the stamp quantum, the atomics' run-to-run noise and the waits on `ev_done`.

Seen on the MI355X: stamp quantum 40 ns; the (1, 0) step run twice differs by 1.0e-7 .. 1.6e-7 in the flat gradient (worst
tensor 0.03 of its bar, dx the same bits).  Edge (i), `ev_ready`, is exercised by every block: the side stream idles until the
event and resumes 17 .. 20 us after it.  Edge (ii), `ev_done`: in the steps of THIS file, enqueued eagerly, the host's launch rate
orders the kernels - at dw_sets = 2 none of the 416 edges of the 12 side-stream steps had its chain launch start within 4 quanta of the
end of the dw it waits for (closest 17 us; 0.4 ms at 6 sets, 0.6 ms at 8) - so what these tests cover of the set rotation is its
index arithmetic and its results.  tests/test_gpu_stalled_schedule.py runs the same matrix with every launch enqueued behind a
stall, where only the events order the kernels: no edge of its 456 (2, 6 and 8 sets) was violated, and the closest stood 17.4 us
(2 sets), 18.1 us (6) and 54.8 us (8) behind the dw's end.  That is the distance of a launch behind any cross-stream event here
(edge (i) shows 16 .. 19 us in the same timelines), so the 4-quanta count of waits stays 0 there too and is asserted nowhere; the
table is in that file's head.
"""
import ctypes as C
import json
import os
import re
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

import ralenet_oracle as O
import schedule_util as S
from parity_util import compare_grads, oracle_trace, oracle_windows, rel, window_grad_errors

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L = 256
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(leads, seed):
    p = O.init_params(O.ralenet_param_shapes("full", leads), seed)
    g = torch.Generator().manual_seed(seed + 1)
    for k in p:
        if "relative_position_bias_table" in k:
            p[k] = 0.3 * torch.randn(p[k].shape, generator=g)
    return p


def _model(leads, max_batch, p32=None, **kw):
    from ecg_denoise_amd import RALENet
    m = RALENet("full", leads=leads, L=L, max_batch=max_batch, device=DEV, **kw)
    if p32 is not None:
        m.load_state_dict(p32, strict=False)
    return m


def _data(B, leads, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, leads, L, generator=g).to(DEV), torch.randn(B, leads, L, generator=g).to(DEV)


def _lib():
    from ecg_denoise_amd import _lib
    return _lib


def _option(m, key, value):
    _lib().check(_lib().lib().ral_set_option(m.eng.h, key.encode(), value))


def _tensors(m):
    return [(e["name"], e["offset"], int(np.prod(e["shape"]))) for e in m.eng.entries if e["kind"] == 0]


def _bar_ratio(m, a, b):
    """per tensor |a - b| / (2e-5 |b| + 1e-9), the bar of test_gpu_configs.py -> {name: ratio} (pass: <= 1)"""
    a, b = a.double(), b.double()
    return {k: (a[o:o + n] - b[o:o + n]).norm().item() / (2e-5 * b[o:o + n].norm().item() + 1e-9) for k, o, n in _tensors(m)}


def _assert_grads(m, got, want, what):
    r = _bar_ratio(m, got, want)
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, (what, bad)


def _step(m, p32, x, t, lanes, side):
    """one train pass from the same parameters and BatchNorm state under the schedule (lanes, side)"""
    S.set_schedule(m, lanes, side)
    m.load_state_dict(p32, strict=False)
    m.eng.state.zero_(); m.eng.state[8:].fill_(1.0)
    m.train()
    y, loss, dx = S.train_pass(m, x, t, want_dx=True)
    torch.cuda.synchronize()
    return {"y": y.clone(), "loss": loss.item(), "dx": dx.clone(), "grads": m.eng.grads.clone(), "state": m.eng.state.clone()}


def _timeline(m, x, t, lanes, side, what):
    rows = S.profiled_step(m, x, t)
    sets = S.expected_sets()
    found, bad = S.check_timeline(rows, lanes, side, sets)
    f = lambda v: "-" if v is None else f"{v * 1e3:.3f}"
    print(f"[schedule] {what}: expected (lanes {lanes}, side {side}, sets {sets}); found lanes {found['lanes']}, chain streams "
          f"{found['chain_streams']}, dw streams {found['dw_streams']}, rows {found['rows']}, quantum {found['quantum_ms'] * 1e6:.1f} ns; "
          f"ev_ready slack min {f(found['slack_ready_ms'])} us; ev_done edges {found['edges_done']}, slack min {f(found['slack_done_ms'])} us, "
          f"waited (within 4 quanta) {found['waits']}; violations {S.names(bad)}")
    assert found["lanes"] == lanes and all(n == 18 * lanes for n in found["counts"].values()), (found, bad)
    if side:      # the two invariants ran over every block of every lane
        assert found["edges_ready"] == 18 * lanes and found["edges_done"] == (18 - sets) * lanes, (found, bad)
    return found, bad


# ---------------------------------------------------------------------------------------------------------------------
# a .. c: one handle of 256 windows, shared (the serialised reference of each batch size is computed once)
# ---------------------------------------------------------------------------------------------------------------------
class _Shared:
    def __init__(self):
        self.p32 = _params(1, 1234)
        self.m = _model(1, 256, self.p32)
        self.x, self.t = _data(256, 1, 2023)
        self.refs = {}

    def ref(self, B):
        """the step at (1 lane, no side stream), and the run-to-run noise of its float atomics"""
        if B not in self.refs:
            x, t = self.x[:B].contiguous(), self.t[:B].contiguous()
            a = _step(self.m, self.p32, x, t, 1, 0)
            b = _step(self.m, self.p32, x, t, 1, 0)
            assert torch.equal(a["y"], b["y"]) and a["loss"] == b["loss"] and torch.equal(a["state"], b["state"])
            r = _bar_ratio(self.m, b["grads"], a["grads"])
            worst = sorted(r.items(), key=lambda kv: -kv[1])[:3]
            print(f"[schedule] noise floor of (1,0) run twice at B={B}: {sum(v > 0 for v in r.values())} of {len(r)} tensors differ; "
                  f"flat gradient rel {rel(b['grads'].cpu().numpy(), a['grads'].cpu().numpy()):.2e}, dx rel "
                  f"{rel(b['dx'].cpu().numpy(), a['dx'].cpu().numpy()):.2e}; worst tensors, as a fraction of the bar 2e-5 |b| + 1e-9: "
                  + ", ".join(f"{k} {v:.3f}" for k, v in worst))
            for k, v in r.items():
                if v > 0:
                    print(f"[schedule]   noise B={B} {k}: {v:.4f} of the bar")
            self.refs[B] = a
        return self.refs[B]


@pytest.fixture(scope="module")
def shared():
    return _Shared()


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("lanes,B", [(1, 256), (2, 256), (2, 130), (3, 192), (4, 256)])
def test_schedule_matrix_equals_the_serialised_step(shared, lanes, B, side):
    """Every (lanes, side stream) against (1, 0) at the same batch on the same handle: the forward bit for bit, the gradients
    within the atomics' bars - and the timeline of a recorded step must show the lanes, the streams and the event edges of the
    schedule that was asked for (a step that silently ran one lane fails here)."""
    m, x, t = shared.m, shared.x[:B].contiguous(), shared.t[:B].contiguous()
    ref = shared.ref(B)
    got = _step(m, shared.p32, x, t, lanes, side)
    assert torch.equal(got["y"], ref["y"])
    assert got["loss"] == ref["loss"]
    assert torch.equal(got["state"], ref["state"])
    assert rel(got["dx"].cpu().numpy(), ref["dx"].cpu().numpy()) < 1e-6
    assert rel(got["grads"].cpu().numpy(), ref["grads"].cpu().numpy()) < 1e-6
    _assert_grads(m, got["grads"], ref["grads"], (lanes, B, side))
    found, bad = _timeline(m, x, t, lanes, side, f"matrix lanes={lanes} B={B} side={side}")
    assert not bad, bad
    assert found["lanes"] == lanes


@pytest.mark.parametrize("lanes,B", [(3, 192), (4, 256)])
def test_lane_boundaries_match_fp64_oracle(shared, lanes, B):
    """dy is zero except on 8 windows around every lane boundary: y on them and every parameter gradient against the fp64 oracle."""
    m, x, t = shared.m, shared.x[:B].contiguous(), shared.t[:B].contiguous()
    per = B // lanes
    idx = [w for b in range(1, lanes) for w in range(b * per - 4, b * per + 4)]
    assert per == 64 and idx[:8] == list(range(60, 68))
    S.set_schedule(m, lanes, 1)
    m.load_state_dict(shared.p32, strict=False)
    m.train()
    y = m(x)
    dy = torch.zeros_like(y)
    ix = torch.tensor(idx, device=DEV)
    dy[ix] = 2.0 * (y[ix] - t[ix]) / (B * L)
    m.backward(dy)
    torch.cuda.synchronize()
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    pred, want = oracle_windows(shared.p32, x.cpu(), t.cpu(), idx)
    assert rel(y[ix].cpu().numpy(), pred.numpy()) < 1e-5
    err = window_grad_errors(m.named_grads(), want)
    print(f"[schedule] lane boundaries lanes={lanes} B={B}: y rel {rel(y[ix].cpu().numpy(), pred.numpy()):.2e}, worst gradient rel "
          f"{max(err.values()):.2e}")
    bad = {k: e for k, e in err.items() if e > 1e-4}
    assert not bad, bad
    found, tb = _timeline(m, x, t, lanes, 1, f"lane boundaries lanes={lanes} B={B}")     # ... and it did run that many lanes
    assert not tb and found["lanes"] == lanes, (found, tb)


@pytest.mark.parametrize("lanes,B,expect", [(3, 192, 3), (3, 190, 1), (3, 189, 1), (3, 64, 1), (4, 255, 1)])
def test_fallback_rule_of_the_lane_split(shared, lanes, B, expect):
    """a batch that is no multiple of the lane count, or has fewer than 64 windows per lane, runs on one lane"""
    m, x, t = shared.m, shared.x[:B].contiguous(), shared.t[:B].contiguous()
    S.set_schedule(m, lanes, 1)
    found, bad = _timeline(m, x, t, expect, 1, f"fallback lanes={lanes} B={B}")
    assert found["lanes"] == expect
    assert not bad, bad


def _plan_entries(backward, B, lanes):
    """the pass as `ral_ralenet_pass_plan` gives it -> [(node kind, lane)] in issue order"""
    lib = _lib().lib()
    row, geom = (C.c_int32 * 9)(), (C.c_int32 * 9)()
    n = lib.ral_ralenet_pass_plan(backward, B, lanes, 0, row, 9)
    assert n > 0, lib.ral_last_error()
    out = []
    for k in range(n):
        assert lib.ral_ralenet_pass_plan(backward, B, lanes, k, row, 9) == n, lib.ral_last_error()
        assert lib.ral_ralenet_node_geom(row[0], geom, 9) > 0, lib.ral_last_error()
        out.append((geom[0], row[1]))
    return out


@pytest.mark.parametrize("lanes,side", [(1, 0), (2, 1), (3, 1)])
def test_timeline_is_the_expansion_of_the_pass_plan(shared, lanes, side):
    """One recorded step of 192 windows: the (kind, stream) sequence of its timeline, in issue order, is the plan's entries
    expanded - a forward stage entry on lane k is 2 x (qkv_fwd, attn_fwd, mlp_fwd) on chain stream k, a resampler entry one
    resample_fwd / resample_bwd, a backward stage entry 2 x (mlp_bwd, attn_bwd, qkv_bwd) on the chain, each followed by its
    dw on the lane's side stream (on the chain without side streams).  The timeline numbers streams by first appearance:
    the chains 0 .. lanes - 1 in the forward, then lane k's side stream as lanes + k (the first stage of the backward issues
    lane 0's blocks, and with them its dw, before lane 1's)."""
    B = 192
    m, x, t = shared.m, shared.x[:B].contiguous(), shared.t[:B].contiguous()
    S.set_schedule(m, lanes, side)
    rows = S.profiled_step(m, x, t)
    want = []
    for kind, k in _plan_entries(0, B, lanes):
        want += [("qkv_fwd", k), ("attn_fwd", k), ("mlp_fwd", k)] * 2 if kind == 0 else [("resample_fwd", k)]
    for kind, k in _plan_entries(1, B, lanes):
        dw = lanes + k if side else k
        want += [("mlp_bwd", k), ("attn_bwd", k), ("qkv_bwd", k), ("dw", dw)] * 2 if kind == 0 else [("resample_bwd", k)]
    got = [(r[0], r[1]) for r in rows]
    assert len(want) == lanes * (9 * 6 + 8 + 9 * 8 + 8)
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), None)
    assert got == want, (first, got[first:first + 4] if first is not None else None, want[first:first + 4] if first is not None else len(got))


# ---------------------------------------------------------------------------------------------------------------------
# d, e: fresh processes
# ---------------------------------------------------------------------------------------------------------------------
def _child(cmd, env, timeout):
    """one child with the GPU open at a time, under a time limit; a child ended by a signal or the limit fails the test"""
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert p.returncode >= 0, f"child ended by signal {-p.returncode}\n" + p.stdout[-2000:] + p.stderr[-2000:]
    return p


@pytest.mark.parametrize("sets", [2, 8])
def test_schedule_tests_under_other_set_counts(sets):
    """tests a .. c of this file again in a fresh process with 2 and with 8 sets of backward temporaries (the switch is latched):
    at 2, block i + 2 of a lane's chain waits for the weight gradients of block i at every block."""
    opts = ",".join(o for o in (os.environ.get("RAL_TEST_OPTIONS", ""), f"dw_sets={sets}") if o)
    p = _child([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-s", "-m", "gpu", "-k",
                "schedule_matrix or lane_boundaries or fallback_rule"], dict(os.environ, RAL_TEST_OPTIONS=opts), 900)
    lines = [ln[ln.index("[schedule]"):] for ln in p.stdout.splitlines() if "[schedule]" in ln and "[schedule]   noise" not in ln]      # (behind pytest's progress dots)
    print("\n".join(ln.replace("[schedule]", f"[schedule] dw_sets={sets}:", 1) for ln in lines))
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    steps = [ln for ln in lines if "expected (lanes" in ln]
    assert len(steps) == 17 and all(f"sets {sets})" in ln for ln in steps)
    edges = [(int(a), float(b), int(c)) for a, b, c in re.findall(r"ev_done edges (\d+), slack min (-?[0-9.]+) us, waited \(within 4 quanta\) (\d+)",
                                                                  "\n".join(steps))]
    print(f"[schedule] dw_sets={sets}: {sum(e[2] for e in edges)} of {sum(e[0] for e in edges)} ev_done edges of {len(edges)} side-stream steps "
          f"had the chain start within 4 quanta of the dw's end; smallest distance {min(e[1] for e in edges):.1f} us")
    assert " passed" in p.stdout and "skipped" not in p.stdout and "deselected" in p.stdout


@pytest.mark.parametrize("var,value,B,lanes,ignored", [("RAL_LANES", "3", 192, 3, False), ("RAL_LANES", "4", 256, 4, False),
                                                       ("RAL_LANES", "5", 256, 2, True), ("RAL_LANES", "x", 256, 2, True),
                                                       ("RAL_NO_SIDE_STREAM", "1", 256, 2, False)])
def test_environment_variables_select_the_schedule(var, value, B, lanes, ignored):
    """the two environment variables the library reads, in fresh processes: a model with the library's defaults, one recorded
    step, the checker's findings as JSON"""
    env = {k: v for k, v in os.environ.items() if k not in ("RAL_LANES", "RAL_NO_SIDE_STREAM")}
    env[var] = value
    p = _child([sys.executable, os.path.join(ROOT, "tests", "schedule_util.py"), str(B)], env, 300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    out = json.loads(next(ln for ln in p.stdout.splitlines() if ln.startswith("SCHEDULE "))[len("SCHEDULE "):])
    print(f"[schedule] {var}={value} B={B}: lanes {out['found']['lanes']}, dw on chain streams {out['dw_on_chain']}, "
          f"violations {out['violations']}")
    assert out["found"]["lanes"] == lanes
    assert not out["violations"]
    assert out["dw_on_chain"] == (var == "RAL_NO_SIDE_STREAM")
    note = [ln for ln in p.stderr.splitlines() if "ignored" in ln and var in ln]
    assert bool(note) == ignored, p.stderr[-2000:]


# ---------------------------------------------------------------------------------------------------------------------
# f: one handle, changing batches
# ---------------------------------------------------------------------------------------------------------------------
def test_changing_batches_on_one_handle(shared):
    """One handle, side streams on, a step per entry: first 256, 5, 192, 130, 64, 256 windows with `lanes` = 4 - by the fallback
    rule these run 4, 1, 1, 1, 1, 4 lanes - then the lane option changed between steps so that the count actually varies:
    (lanes, B) = (3, 192), (2, 130), (4, 64), (2, 256), (4, 256), (3, 192), (1, 256), (4, 256) run 3, 2, 1, 2, 4, 3, 1, 4 lanes.
    After each step y and the gradients are those of a fresh one-lane handle of exactly that batch: nothing of the previous
    step's lanes, sets or pending flags is left over."""
    p32 = shared.p32
    m = _model(1, 256, p32)
    m.train()
    refs = {}
    plan = [(4, B) for B in (256, 5, 192, 130, 64, 256)] + [(3, 192), (2, 130), (4, 64), (2, 256), (4, 256), (3, 192), (1, 256), (4, 256)]
    for lanes, B in plan:
        x, t = shared.x[:B].contiguous(), shared.t[:B].contiguous()
        if B not in refs:
            f = _model(1, B, p32)
            refs[B] = _step(f, p32, x, t, 1, 0)
            del f
        S.set_schedule(m, lanes, 1)
        y, loss, _ = S.train_pass(m, x, t)
        torch.cuda.synchronize()
        assert torch.equal(y, refs[B]["y"]), (lanes, B)
        assert loss.item() == refs[B]["loss"], (lanes, B)
        _assert_grads(m, m.eng.grads, refs[B]["grads"], (lanes, B))


@pytest.mark.parametrize("lanes,B", [(1, 256), (3, 192), (4, 256)])
def test_gradient_maxima_have_one_slot_per_block_and_lane(shared, lanes, B):
    """`gmax + (bi * 4 + lane) * 4`: the wide blocks whose split kernels publish the largest |dx2|, |du|, |dx1|, |dqkv| of a lane's
    windows (the scales of its weight-gradient products) write the slot of their own lane.  The workspace tensor is read
    back after the backward (it is zeroed at the start of the next one): slots of lanes that ran are positive, all others zero;
    and with dy scaled by 8^lane the slots of lane k grow by 8^k, so a shared or mis-strided slot cannot hide.  The backward
    of a lane is linear in its dy and a power of two changes no fp32 mantissa; the bar is 1e-5 per slot all the same - the
    project's bar for this linearity is 2e-6 in L2 (test_backward_is_linear_in_the_output_gradient_over_sixteen_decades), a
    maximum is a single element of such a tensor, and the factors to be told apart are 8."""
    m, x, t = shared.m, shared.x[:B].contiguous(), shared.t[:B].contiguous()
    S.set_schedule(m, lanes, 1)
    m.load_state_dict(shared.p32, strict=False)
    m.train()
    y = m(x)
    dy = 2.0 * (y - t) / (B * L)
    per = B // lanes
    factor = torch.tensor([8.0 ** k for k in range(lanes)], device=DEV)
    res = []
    for scale in (torch.ones(B, device=DEV), factor.repeat_interleave(per)):
        m.backward(dy * scale[:, None, None])
        torch.cuda.synchronize()
        res.append(m.debug_tensor("gmax")[:18 * 4 * 4].view(18, 4, 4).clone())
    g0, g1 = res
    assert torch.isfinite(g0).all() and (g0 >= 0).all()
    pub = [bi for bi in range(18) if g0[bi].abs().sum().item() > 0]
    print(f"[schedule] gmax lanes={lanes} B={B}: blocks that publish maxima {pub}; lane 0 of block {pub[0] if pub else None}: {g0[pub[0], 0].tolist() if pub else None}")
    assert pub and set(pub) <= set(range(6, 14)), pub          # the two wide levels
    for bi in pub:
        assert (g0[bi, :lanes] > 0).all(), (bi, g0[bi])
        assert (g0[bi, lanes:] == 0).all(), (bi, g0[bi])
    want = g0[pub][:, :lanes].double() * factor[None, :, None].double()
    dev = ((g1[pub][:, :lanes].double() - want).abs() / want).max().item()
    print(f"[schedule] gmax lanes={lanes} B={B}: largest deviation of a slot from 8^lane x its unscaled value {dev:.2e}")
    assert dev <= 1e-5, (g1[pub], g0[pub])
    assert (g1[pub][:, lanes:] == 0).all()


@pytest.mark.parametrize("lanes,B", [(3, 192), (4, 256)])
def test_early_gradient_bucket_after_a_one_lane_step(shared, lanes, B):
    """the decoder's gradients are final when bucket 1's events have fired - with 3 and 4 lanes (each lane records its own pair
    of events), straight after a step that ran one lane (`dec_lanes` of that step must not be what is waited for)"""
    from ecg_denoise_amd.dp import HipEngineAdapter
    m = _model(1, 256, shared.p32)
    S.set_schedule(m, lanes, 1)
    m.train()
    e = HipEngineAdapter(m)
    (o0, n0), (o1, n1) = e.grad_buckets()
    assert o0 == 0 and o1 == n0 and o1 + n1 == m.eng.grads.numel() and n1 > 0
    for _ in range(2):
        S.train_pass(m, shared.x[:5].contiguous(), shared.t[:5].contiguous())      # one lane
        x, t = shared.x[:B].contiguous(), shared.t[:B].contiguous()
        e.forward_begin(x); pred = e.forward_end(B)
        e.loss(pred, t, B)
        e.backward_begin()
        comm = e.bucket_stream()
        e.bucket_wait(1, comm)
        with torch.cuda.stream(comm):
            early = m.eng.grads[o1:o1 + n1].clone()
        e.backward_end(B)
        e.bucket_wait(0, comm)
        with torch.cuda.stream(comm):
            late = m.eng.grads[:o1].clone()
        torch.cuda.synchronize()
        assert early.abs().sum().item() > 0
        assert torch.equal(early, m.eng.grads[o1:o1 + n1])
        assert torch.equal(late, m.eng.grads[:o1])
    _assert_grads(m, m.eng.grads, shared.ref(B)["grads"], (lanes, B))


# ---------------------------------------------------------------------------------------------------------------------
# g: the weight planes an eval-mode model keeps (static_params / planes_valid / skip_prep / prep_stale)
# ---------------------------------------------------------------------------------------------------------------------
class _Cache:
    def __init__(self):
        self.p1, self.p2 = _params(2, 1234), _params(2, 4321)
        self.x, self.t = _data(128, 2, 7)

    def fresh_eval(self, sd, x, **kw):
        """a new handle holding `sd`, in eval mode -> its output for x"""
        f = _model(2, x.shape[0], **kw)
        if sd is not None:
            f.load_state_dict(sd, strict=False)
        f.eval()
        y = f(x).clone()
        torch.cuda.synchronize()
        return y


@pytest.fixture(scope="module")
def cache():
    return _Cache()


@pytest.mark.parametrize("B", [4, 128])
def test_eval_forward_after_load_state_dict_uses_the_new_weights(cache, B):
    x = cache.x[:B].contiguous()
    m = _model(2, B, cache.p1)
    m.eval()
    y1 = m(x).clone()
    m.load_state_dict(cache.p2, strict=False)
    y2 = m(x).clone()
    assert not torch.equal(y1, y2)
    assert torch.equal(y2, cache.fresh_eval(cache.p2, x))
    assert torch.equal(m(x), y2)                       # ... and the forward that skips the preparation gives the same bits


@pytest.mark.parametrize("B", [4, 128])
def test_eval_forward_after_train_steps_uses_the_stepped_weights(cache, B):
    x, t = cache.x[:B].contiguous(), cache.t[:B].contiguous()
    m = _model(2, B, cache.p1)
    m.eval()
    y0 = m(x).clone()
    m.train()
    m.train_step(x, t); m.train_step(x, t)
    m.eval()
    y = m(x).clone()
    assert not torch.equal(y, y0)
    assert torch.equal(y, cache.fresh_eval(m.state_dict(), x))


def test_eval_forwards_of_changing_batch_keep_the_planes(cache):
    x = cache.x
    m = _model(2, 128, cache.p1)
    m.eval()
    want = {128: cache.fresh_eval(cache.p1, x), 3: cache.fresh_eval(cache.p1, x[:3].contiguous())}
    got = [m(x[:B].contiguous()).clone() for B in (128, 3, 128)]
    for B, y in zip((128, 3, 128), got):
        assert torch.equal(y, want[B]), B
    _option(m, "side_stream", 0)                       # the preparation inline, in front of the lanes
    for B in (128, 3, 128):
        assert torch.equal(m(x[:B].contiguous()), want[B]), ("inline", B)


def test_eval_forward_after_reset_parameters(cache):
    x = cache.x[:4].contiguous()
    m = _model(2, 4, cache.p1)
    m.eval()
    y1 = m(x).clone()
    m.reset_parameters(77)
    y2 = m(x).clone()
    assert not torch.equal(y1, y2)
    assert torch.equal(y2, cache.fresh_eval(None, x, seed=77))


def test_in_place_edit_needs_params_changed_in_eval_mode_only(cache):
    """the contract of `_params_changed`: an eval-mode model is told about an in-place edit; a training-mode model sees it"""
    key = "transformer.blocks.0.attn.qkv_proj.to_q.weight"     # a wide-level matrix: the projection reads its fp16 planes
    x = cache.x[:4].contiguous()
    m = _model(2, 4, cache.p1)
    m.eval()
    y1 = m(x).clone()
    dict(m.named_parameters())[key].mul_(1.5)
    m._params_changed()
    y2 = m(x).clone()
    assert not torch.equal(y1, y2)
    assert torch.equal(y2, cache.fresh_eval(m.state_dict(), x))
    m.train()
    dict(m.named_parameters())[key].mul_(0.5)
    y3 = m(x).clone()
    f = _model(2, 4, m.state_dict())
    f.train()
    assert torch.equal(y3, f(x))


def test_option_set_between_forward_and_backward(cache):
    x, t = cache.x[:4].contiguous(), cache.t[:4].contiguous()
    m = _model(2, 4, cache.p1)
    m.train()
    S.train_pass(m, x, t)
    torch.cuda.synchronize()
    g0 = m.eng.grads.clone()
    y = m(x); m.loss_and_metrics(y, t)
    _option(m, "side_stream", 1)                       # the value it has: the planes queued by the forward count as stale
    m.backward()
    torch.cuda.synchronize()
    _assert_grads(m, m.eng.grads, g0, "side_stream set again")
    # the forward on fp16-pair products, the backward on fp32 MFMA: its transposes and scales are formed again
    _option(m, "f16_split", 64)
    y = m(x); m.loss_and_metrics(y, t)
    _option(m, "f16_split", 0)
    m.backward()
    torch.cuda.synchronize()
    p = OrderedDict((k, v.double().requires_grad_(True)) for k, v in cache.p1.items())
    yo, _ = oracle_trace(p, x.cpu().double(), "full", O.new_bn_state(8, torch.float64))
    grads = torch.autograd.grad(O.mse(yo, t.cpu().double()), list(p.values()), allow_unused=True)
    err = compare_grads(m.named_grads(), p, grads)
    bad = {k: v for k, v in err.items() if v > (1e-5 if k.startswith("gradabs:") else 1e-4)}
    assert not bad, bad


def test_second_backward_of_one_forward(cache):
    x, t = cache.x[:4].contiguous(), cache.t[:4].contiguous()
    m = _model(2, 4, cache.p1)
    m.train()
    S.train_pass(m, x, t)
    torch.cuda.synchronize()
    g1, dy = m.eng.grads.clone(), m._dy.clone()
    m.backward(dy)                                     # the transposes prepared under the forward are consumed: formed again
    torch.cuda.synchronize()
    _assert_grads(m, m.eng.grads, g1, "second backward")


# ---------------------------------------------------------------------------------------------------------------------
# h: profile hooks
# ---------------------------------------------------------------------------------------------------------------------
def test_profile_hooks(shared):
    lib, chk = _lib().lib(), _lib().check
    m, h = shared.m, shared.m.eng.h
    assert lib.ral_profile_select(h, b"attn_sideways") != 0
    assert "unknown kernel kind attn_sideways" in lib.ral_last_error().decode()
    ms, n = C.c_double(), C.c_int64()
    m.eval()
    for lanes in (1, 2):
        S.set_schedule(m, lanes, 1)
        chk(lib.ral_profile_select(h, b"attn_fwd"))
        m(shared.x)
        chk(lib.ral_profile_read(h, C.byref(ms), C.byref(n)))
        assert n.value == 18 * lanes and ms.value > 0.0
        chk(lib.ral_profile_read(h, C.byref(ms), C.byref(n)))
        assert n.value == 0 and ms.value == 0.0
    chk(lib.ral_profile_select(h, b"*"))
    m(shared.x)
    rows = (C.c_double * (4 * 4096))()
    assert lib.ral_profile_timeline(h, rows, 3, C.byref(n)) != 0
    want = (3 * 18 + 8) * 2                            # per lane: three launches per block and the eight resamplers
    assert n.value == want
    err = lib.ral_last_error().decode()
    assert "timeline" in err and f"{want} rows" in err
    got = S.read_timeline(m)
    assert len(got) == want and {r[0] for r in got} == {"qkv_fwd", "attn_fwd", "mlp_fwd", "resample_fwd"}
    chk(lib.ral_profile_select(h, b""))
    m.train()
    S.train_pass(m, shared.x, shared.t)
    torch.cuda.synchronize()
    chk(lib.ral_profile_read(h, C.byref(ms), C.byref(n)))
    assert n.value == 0
    assert S.read_timeline(m) == []
