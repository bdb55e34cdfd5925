"""The RA-LENet step's event edges while they bind (`pytest -m gpu`): the schedule matrix of tests/test_gpu_schedule.py again,
each step enqueued on a stream S of the caller's behind a bounded stall (tests/stall_util.py).  The host has finished
enqueueing before the device runs anything, so from the end of the stall on only the events order the kernels:

  * entry - x and t are NaN until a copy on S behind the stall fills them, and the parameter buffer is rewritten there too: the
    lanes' `ev_fork`, the side streams' fork behind `k_zero_bwd` and the preparation stream's `ev_prep_go` are needed for the
    step to read them;
  * exit - y, the loss, dx, the gradients and the BatchNorm state are cloned on S directly after the call that produces them,
    and only S is synchronised: `join_lanes` and the side streams' `ev_join` are needed for the clones to be complete;
  * in between - `ev_ready` / `ev_done` are read off the recorded timeline by schedule_util.check_timeline.

Seen on the MI355X (one run, one recorded step per case; sleep kernel calibrated at 2.39e6 cycles per ms; every case reported
`pending` True, no timeline had a violation, every value assert held).  enq: wall-clock time of the host to enqueue the body;
stall: asked / achieved; body: gate -> end of the body on the device; edges / slack / waits: `edges_done`, the smallest
`slack_done_ms` and `waits` (chain launches that started within 4 quanta = 160 ns of the end of the dw they wait for) of
check_timeline; busy: the least busy chain stream (stall_util.stream_gaps).

    sets  lanes  B    side  enq ms  stall ms     body ms  edges  slack us  waits  busy
    6     1      256  0      1.36   20.0 / 19.9   4.42      0      -        0     0.79
    6     1      256  1      1.67   20.0 / 20.0   4.95     12    925.5      0     0.50
    6     2      256  1      3.14   20.0 / 19.9   4.17     24    526.7      0     0.69
    6     2      130  1      3.01   20.0 / 19.9   4.80     24     18.1      0     0.46
    6     3      192  1      4.31   20.0 / 20.0   9.71     36   1920.6      0     0.21
    6     4      256  1      6.04   24.1 / 24.1   9.01     48   1413.5      0     0.26
    2     1      256  0      1.34   20.0 / 19.9   4.39      0      -        0     0.79
    2     1      256  1      1.03   20.0 / 20.0   4.91     16    191.1      0     0.50
    2     2      256  1      2.05   20.0 / 19.9   4.22     32     33.3      0     0.68
    2     2      130  1      1.96   20.0 / 19.9   4.74     32     17.4      0     0.46
    2     3      192  1      2.76   20.0 / 20.0   9.69     48    537.6      0     0.21
    2     4      256  1      3.68   20.0 / 20.0   8.94     64    381.2      0     0.27
    8     1      256  0      1.34   20.0 / 19.9   4.45      0      -        0     0.79
    8     1      256  1      1.67   20.0 / 20.0   4.92     10   1347.6      0     0.51
    8     2      256  1      3.26   20.0 / 19.9   4.27     20    892.3      0     0.69
    8     2      130  1      3.08   20.0 / 19.9   4.77     20     54.8      0     0.46
    8     3      192  1      4.56   20.0 / 20.0   9.67     30   2774.3      0     0.22
    8     4      256  1     10.28   41.1 / 41.1   8.91     40   2005.3      0     0.26

`ev_done`: by the rule `waits` counts (within 4 quanta) NO edge bound, at any set count: 0 of 192 edges at 2 sets, 0 of 144 at 6, 0
of 120 at 8, so no case asserts `waits >= 1` (BINDS_AT_TWO_SETS is empty) and the count stays printed.  The closest edges, 17.4 us
(2 sets, 2 lanes, B = 130), 18.1 us (6 sets, same case) and 33.3 us (2 sets, 2 lanes, B = 256), are as far from the dw's end as a
launch behind ANY cross-stream event is from its event on this machine: `ev_ready`, which binds at every block by construction,
shows 16.1 .. 19.2 us as its smallest distance in the same timelines.  A chain launch that had to wait for `ev_done` therefore
cannot start within 160 ns of it, and those closest edges very probably did wait; the rule cannot tell.  What the stalled steps
do establish for this edge: with every launch enqueued before the device starts, no block of any lane started before the dw
that read its set of temporaries had ended (a violation is a distance below -40 ns; the smallest seen is +17.4 us), and the
gradients are those of the serialised step.

Bench shape ("full", 2 leads, L = 512, B = 2048, default schedule, no stall): no violation; 24 `ev_done` edges, smallest slack 1202.6 us,
waits 0; `ev_ready` smallest distance 17.5 us; chain streams busy 0.66 and 0.90 of their span (median gap between launches 7 us),
the side streams 0.31 and 0.55.  Early bucket behind the stall: lanes 3 / 4, host enqueue 2.91 / 3.60 ms, stall 20.0 / 19.9 ms
achieved, body 6.43 / 7.17 ms, `early` and `late` bit for bit.
"""
import os
import re
import sys

import pytest
import torch

import schedule_util as S
import stall_util as U
from parity_util import rel
from test_gpu_schedule import DEV, _Shared, _assert_grads, _child, _lib, _model, _params

pytestmark = pytest.mark.gpu

CASES = [(1, 256, 0), (1, 256, 1), (2, 256, 1), (2, 130, 1), (3, 192, 1), (4, 256, 1)]
# (lanes, B, side) whose stalled step showed waits >= 4 on the MI355X at dw_sets = 2: from then on `ev_done` must bind there
BINDS_AT_TWO_SETS = set()


@pytest.fixture(scope="module")
def shared():
    return _Shared()


def _report(rows, lanes, side, what):
    sets = S.expected_sets()
    found, bad = S.check_timeline(rows, lanes, side, sets)
    f = lambda v: "-" if v is None else f"{v * 1e3:.3f}"
    busy = U.least_busy(rows, found["chain_streams"])
    print(f"[schedule] {what}: expected (lanes {lanes}, side {side}, sets {sets}); found lanes {found['lanes']}, chain streams "
          f"{found['chain_streams']}, dw streams {found['dw_streams']}, rows {found['rows']}, quantum {found['quantum_ms'] * 1e6:.1f} ns; "
          f"ev_ready slack min {f(found['slack_ready_ms'])} us; ev_done edges {found['edges_done']}, slack min {f(found['slack_done_ms'])} us, "
          f"waited (within 4 quanta) {found['waits']}; least busy chain {busy:.2f}; violations {S.names(bad)}")
    return found, bad


@pytest.mark.parametrize("lanes,B,side", CASES)
def test_stalled_matrix_equals_the_serialised_step(shared, lanes, B, side):
    """test_schedule_matrix_equals_the_serialised_step with the step queued behind the stall on a stream of the caller's: the
    reference is the eager (1, 0) step at the same batch; inputs and parameters appear on S behind the stall, the results are
    cloned on S, only S is synchronised; the recorded step is the stalled one."""
    m = shared.m
    ref = shared.ref(B)                                                # eager, as today (synchronises the device)
    x0, t0 = shared.x[:B].contiguous(), shared.t[:B].contiguous()
    lib, h = _lib().lib(), m.eng.h
    St = torch.cuda.Stream()
    with torch.cuda.stream(St):
        S.set_schedule(m, lanes, side)
        m.load_state_dict(shared.p32, strict=False)
        m.train()
        flat = m.eng.params.clone()
        state0 = torch.zeros_like(m.eng.state); state0[8:].fill_(1.0)
        x, t = torch.empty_like(x0), torch.empty_like(t0)
    St.synchronize()

    def before():
        for buf in (x, t, m.eng.params, m.eng.state):
            U.poison(buf)
        _lib().check(lib.ral_profile_select(h, b"*"))                   # every kind, as S.profiled_step selects them

    def body():
        U.late(x, x0); U.late(t, t0); U.late(m.eng.state, state0)
        U.late(m.eng.params, flat)
        m._params_changed()
        y = m(x)
        yc = y.clone()
        loss, _, _ = m.loss_and_metrics(y, t)
        lc = loss.clone()
        dx = m.backward(want_dx=True)
        return {"y": yc, "loss": lc, "dx": dx.clone(), "grads": m.eng.grads.clone(), "state": m.eng.state.clone()}

    what = f"stalled matrix lanes={lanes} B={B} side={side} sets={S.expected_sets()}"
    got, st, _ = U.run_stalled(St, body, what, before)
    rows = S.read_timeline(m)
    _lib().check(lib.ral_profile_select(h, b""))
    found, bad = _report(rows, lanes, side, what)
    assert st.pending is True
    for k, v in got.items():
        assert not torch.isnan(v).any(), k
    assert torch.equal(got["y"], ref["y"])
    assert got["loss"].item() == ref["loss"]
    assert torch.equal(got["state"], ref["state"])
    assert rel(got["dx"].cpu().numpy(), ref["dx"].cpu().numpy()) < 1e-6
    assert rel(got["grads"].cpu().numpy(), ref["grads"].cpu().numpy()) < 1e-6
    _assert_grads(m, got["grads"], ref["grads"], (lanes, B, side))
    assert not bad, bad
    assert found["lanes"] == lanes and all(n == 18 * lanes for n in found["counts"].values()), (found, bad)
    if side:
        sets = S.expected_sets()
        assert found["edges_ready"] == 18 * lanes and found["edges_done"] == (18 - sets) * lanes, (found, bad)
        if sets == 2 and (lanes, B, side) in BINDS_AT_TWO_SETS:
            assert found["waits"] >= 1, found


@pytest.mark.parametrize("sets", [2, 8])
def test_stalled_matrix_under_other_set_counts(sets):
    """the stalled matrix again in a fresh process with 2 and with 8 sets of backward temporaries (the switch is latched): at 2
    sets block i + 2 of a lane's chain waits for the weight gradients of block i at every block"""
    opts = ",".join(o for o in (os.environ.get("RAL_TEST_OPTIONS", ""), f"dw_sets={sets}") if o)
    p = _child([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-s", "-m", "gpu", "-k", "stalled_matrix_equals"],
               dict(os.environ, RAL_TEST_OPTIONS=opts), 600)
    tag = lambda name: [ln[ln.index(name):] for ln in p.stdout.splitlines() if name in ln and "[schedule]   noise" not in ln]
    lines = tag("[schedule]")
    print("\n".join(ln.replace("[", f"[dw_sets={sets}] [", 1) for ln in tag("[stall]") + lines))
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    steps = [ln for ln in lines if "expected (lanes" in ln]
    assert len(steps) == len(CASES) and all(f"sets {sets})" in ln for ln in steps)
    assert len([ln for ln in tag("[stall]") if "pending True" in ln]) == len(CASES)
    edges = [(int(a), float(b), int(c)) for a, b, c in re.findall(r"ev_done edges (\d+), slack min (-?[0-9.]+) us, waited \(within 4 quanta\) (\d+)",
                                                                  "\n".join(ln for ln in steps if "side 1" in ln))]
    assert len(edges) == len([c for c in CASES if c[2]])
    print(f"[schedule] stalled, dw_sets={sets}: {sum(e[2] for e in edges)} of {sum(e[0] for e in edges)} ev_done edges of {len(edges)} side-stream steps "
          f"had the chain start within 4 quanta of the dw's end; smallest distance {min(e[1] for e in edges):.1f} us")
    assert " passed" in p.stdout and "skipped" not in p.stdout and "deselected" in p.stdout


def test_bench_shape_timeline_has_no_violations():
    """("full", 2 leads, L = 512, B = 2048), the default schedule, no stall: the device leads at this batch, and the checker
    looks at one recorded step of it"""
    from ecg_denoise_amd import RALENet
    B = 2048
    m = RALENet("full", leads=2, L=512, max_batch=B, device=DEV)
    m.load_state_dict(_params(2, 1234), strict=False)
    g = torch.Generator().manual_seed(2023)
    x = torch.randn(B, 2, 512, generator=g).to(DEV); t = torch.randn(B, 2, 512, generator=g).to(DEV)
    rows = S.profiled_step(m, x, t)
    found, bad = _report(rows, 2, 1, f"bench shape B={B} leads=2 L=512, default schedule, no stall")
    gaps = U.stream_gaps(rows)
    print("[schedule] bench shape, per stream (rows, busy, median gap us): "
          + ", ".join(f"{s}: ({v['rows']}, {v['busy']:.2f}, {v['median_gap_ms'] * 1e3:.1f})" for s, v in sorted(gaps.items())))
    assert not bad, bad
    assert found["lanes"] == 2 and found["dw_streams"] and not set(found["dw_streams"]) & set(found["chain_streams"])
    assert found["edges_ready"] == 36 and found["edges_done"] == (18 - S.expected_sets()) * 2


@pytest.mark.parametrize("lanes,B", [(3, 192), (4, 256)])
def test_early_gradient_bucket_behind_the_stall(shared, lanes, B):
    """test_early_gradient_bucket_after_a_one_lane_step with forward_begin .. backward_begin, `bucket_wait(1, comm)` and the clone on
    `comm` all enqueued behind the stall on S: `comm` really races the encoder's backward, and the decoder's gradients it
    clones are the final ones bit for bit (`early`), as are the encoder's after `bucket_wait(0, comm)` (`late`)"""
    from ecg_denoise_amd.dp import HipEngineAdapter
    St = torch.cuda.Stream()
    x0, t0 = shared.x[:B].contiguous(), shared.t[:B].contiguous()
    x5, t5 = shared.x[:5].contiguous(), shared.t[:5].contiguous()
    with torch.cuda.stream(St):
        m = _model(1, 256, shared.p32)
        S.set_schedule(m, lanes, 1)
        m.train()
        e = HipEngineAdapter(m)
        (o0, n0), (o1, n1) = e.grad_buckets()
        comm = e.bucket_stream()
        x, t = torch.empty_like(x0), torch.empty_like(t0)
    St.synchronize()
    assert o0 == 0 and o1 == n0 and o1 + n1 == m.eng.grads.numel() and n1 > 0

    def before():
        U.poison(x); U.poison(t)

    def body():
        S.train_pass(m, x5, t5)                                        # one lane
        U.late(x, x0); U.late(t, t0)
        e.forward_begin(x); pred = e.forward_end(B)
        e.loss(pred, t, B)
        e.backward_begin()
        e.bucket_wait(1, comm)
        with torch.cuda.stream(comm):
            early = m.eng.grads[o1:o1 + n1].clone()
        e.backward_end(B)
        e.bucket_wait(0, comm)
        with torch.cuda.stream(comm):
            late = m.eng.grads[:o1].clone()
        St.wait_stream(comm)                                           # (the clones are read after S alone has been synchronised)
        return early, late, m.eng.grads.clone()

    (early, late, final), st, _ = U.run_stalled(St, body, f"early bucket lanes={lanes} B={B}", before)
    assert st.pending is True
    assert early.abs().sum().item() > 0
    assert torch.equal(early, final[o1:o1 + n1])
    assert torch.equal(late, final[:o1])
    _assert_grads(m, final, shared.ref(B)["grads"], (lanes, B))
