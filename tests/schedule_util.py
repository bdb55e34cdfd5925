"""Reads the schedule of one RA-LENet train step off the library's own event timeline (`ral_profile_select(h, "*")` /
`ral_profile_timeline`): which streams carried the micro-batch lanes, where the weight-gradient launches ran, and whether
the two event edges between a lane's chain and its weight-gradient stream held.

`check_timeline(rows, lanes, side, sets)` is pure Python (tests/test_schedule_cpu.py feeds it synthetic timelines); the
helpers below it drive a model on the GPU and are imported by tests/test_gpu_schedule.py.  Run as a program,

    python tests/schedule_util.py B

creates a model with the library's defaults (RAL_LANES / RAL_NO_SIDE_STREAM are read by the library at creation), records
one train step of B windows and prints what the checker found as one JSON line: the child processes of the
environment-variable test.

Event stamps are quantised: the checker allows one quantum, taken from the timeline itself (the smallest non-zero
difference between any two of its stamps).  On the MI355X that value was 40 ns for every timeline with more than one
stream (39.6 .. 40.1 after the float32 milliseconds of hipEventElapsedTime; 80 ns twice); a one-lane step without side
streams has all its stamps on one stream, where the end of a launch and the start of the next coincide, and showed
0.6 .. 5 us (see the `[schedule]` lines of tests/test_gpu_schedule.py).
"""
import json
import os
import sys

KINDS = ["qkv_fwd", "attn_fwd", "mlp_fwd", "mlp_bwd", "attn_bwd", "qkv_bwd", "dw", "resample_fwd", "resample_bwd", "stem"]
PER_BLOCK = ("qkv_fwd", "attn_fwd", "mlp_fwd", "mlp_bwd", "attn_bwd", "qkv_bwd", "dw")   # one launch per block and lane
CHAIN = tuple(k for k in KINDS if k not in ("dw", "stem"))                                # kinds that only a lane's chain issues
BLOCKS = 18

# names of the violations
COUNT = "count"              # a per-block kind does not have 18 * lanes rows
LANES = "lanes"              # the attention forward ran on another number of streams
DW_STREAM = "dw_stream"      # weight-gradient rows on the wrong kind of stream
EV_READY = "ev_ready"        # (i)   a dw started before its qkv_bwd ended
EV_DONE = "ev_done"          # (ii)  a chain reused a set of temporaries before the dw reading it ended
OVERLAP = "overlap"          # (iii) two rows of one stream overlap


def _kind(k):
    return k if isinstance(k, str) else KINDS[int(k)]


def quantum(rows):
    """smallest non-zero difference between any two stamps of the timeline (0.0 if there is none)"""
    st = sorted({float(r[2]) for r in rows} | {float(r[3]) for r in rows})
    d = [b - a for a, b in zip(st, st[1:]) if b > a]
    return min(d) if d else 0.0


def check_timeline(rows, lanes, side, sets, near=4):
    """rows: (kind, stream, t0, t1) in issue order, kind a name or an index into KINDS; (lanes, side, sets): the schedule the
    step should have run.  -> (found, violations): `found` is a dict of what the timeline shows, `violations` a list of
    (name, text).  `found["waits"]`: how many chain launches started within `near` quanta of the end of the dw they had to
    wait for (edge (ii) was actually exercised), `found["slack_done_ms"]` the smallest such distance."""
    rows = [(_kind(k), int(s), float(t0), float(t1)) for k, s, t0, t1 in rows]
    q = quantum(rows)
    bad = []
    by_kind = {k: [r for r in rows if r[0] == k] for k in KINDS}
    chain_streams = []                       # in order of first appearance: lane 0 first (it is issued first)
    for r in by_kind["attn_fwd"] or by_kind["attn_bwd"]:
        if r[1] not in chain_streams:
            chain_streams.append(r[1])
    any_chain = {r[1] for r in rows if r[0] in CHAIN}
    dw_streams = sorted({r[1] for r in by_kind["dw"]})
    found = {"lanes": len(chain_streams), "chain_streams": chain_streams, "dw_streams": dw_streams, "quantum_ms": q,
             "counts": {k: len(by_kind[k]) for k in PER_BLOCK}, "rows": len(rows)}
    if len(chain_streams) != lanes:
        bad.append((LANES, f"attention forward on {len(chain_streams)} stream(s) {chain_streams}, expected {lanes}"))
    for k in PER_BLOCK:
        if len(by_kind[k]) != BLOCKS * lanes:
            bad.append((COUNT, f"{len(by_kind[k])} {k} rows, expected {BLOCKS * lanes}"))
    # pairing: a dw row belongs to the nearest qkv_bwd row before it in issue order; that row's stream is the lane
    groups = {}                              # chain stream -> [[mlp_bwd, attn_bwd, qkv_bwd, dw], ...], one per block of its backward
    last_qkv = None
    for r in rows:
        if r[0] in ("mlp_bwd", "attn_bwd", "qkv_bwd"):
            g = groups.setdefault(r[1], [])
            i = ("mlp_bwd", "attn_bwd", "qkv_bwd").index(r[0])
            if r[0] == "mlp_bwd" or not g or g[-1][i] is not None:
                g.append([None, None, None, None])
            g[-1][i] = r
            if r[0] == "qkv_bwd":
                last_qkv = r
        elif r[0] == "dw":
            if last_qkv is None:
                bad.append((EV_READY, f"a dw row (stream {r[1]}) with no qkv_bwd before it"))
                continue
            g = groups[last_qkv[1]]
            if g[-1][2] is not last_qkv or g[-1][3] is not None:
                bad.append((COUNT, f"dw rows and qkv_bwd rows of stream {last_qkv[1]} do not pair up"))
                continue
            g[-1][3] = r
    side_of = {}                             # chain stream -> streams of its dw rows
    for c, g in groups.items():
        side_of[c] = sorted({b[3][1] for b in g if b[3] is not None})
    found["dw_of_lane"] = {str(c): v for c, v in side_of.items()}
    if side:
        on_chain = [r for r in by_kind["dw"] if r[1] in any_chain]
        if on_chain:
            bad.append((DW_STREAM, f"{len(on_chain)} dw rows on chain stream(s) {sorted({r[1] for r in on_chain})} while side streams are expected"))
        elif len(dw_streams) != lanes:
            bad.append((DW_STREAM, f"dw rows on {len(dw_streams)} side stream(s) {dw_streams}, expected one per lane ({lanes})"))
        for c, v in side_of.items():
            if len(v) > 1:
                bad.append((DW_STREAM, f"the dw rows of lane stream {c} sit on several streams {v}"))
    else:
        off = [(c, v) for c, v in side_of.items() if v and v != [c]]
        if off:
            bad.append((DW_STREAM, f"dw rows off their lane's chain stream (lane stream, dw streams): {off}"))
    # causal invariants of the side-stream schedule
    waits, slack_ready, slack_done, edges_done, edges_ready = 0, None, None, 0, 0
    if side:
        for c, g in groups.items():
            for j, b in enumerate(g):
                if b[2] is None or b[3] is None:
                    continue
                d = b[3][2] - b[2][3]                                   # (i) dw[j].t0 - qkv_bwd[j].t1
                edges_ready += 1
                slack_ready = d if slack_ready is None else min(slack_ready, d)
                if d < -q:
                    bad.append((EV_READY, f"lane stream {c} block {j}: dw starts {-d * 1e3:.3f} us before its qkv_bwd ends"))
                if j + sets < len(g) and g[j + sets][0] is not None:
                    d = g[j + sets][0][2] - b[3][3]                     # (ii) mlp_bwd[j + sets].t0 - dw[j].t1
                    edges_done += 1
                    slack_done = d if slack_done is None else min(slack_done, d)
                    if d <= near * q:
                        waits += 1
                    if d < -q:
                        bad.append((EV_DONE, f"lane stream {c}: block {j + sets} starts {-d * 1e3:.3f} us before the dw of block {j} "
                                             f"(same set of temporaries, {sets} sets) ends"))
    found.update(waits=waits, edges_ready=edges_ready, edges_done=edges_done, slack_ready_ms=slack_ready, slack_done_ms=slack_done)
    if side and (edges_ready != BLOCKS * lanes or edges_done != (BLOCKS - sets) * lanes):    # the invariants ran over every block
        bad.append((COUNT, f"{edges_ready} ev_ready and {edges_done} ev_done edges could be checked, expected {BLOCKS * lanes} and "
                           f"{(BLOCKS - sets) * lanes}"))
    # (iii) rows of one stream do not overlap
    last = {}
    for r in rows:
        p = last.get(r[1])
        if p is not None and r[2] < p[3] - q:
            bad.append((OVERLAP, f"stream {r[1]}: {r[0]} starts {(p[3] - r[2]) * 1e3:.3f} us before the {p[0]} issued before it ends"))
        if r[3] < r[2] - q:
            bad.append((OVERLAP, f"stream {r[1]}: a {r[0]} row ends before it starts"))
        last[r[1]] = r
    return found, bad


def names(violations):
    return sorted({n for n, _ in violations})


def expected_sets():
    """the set count of this process: RAL_TEST_OPTIONS (tests/conftest.py hands it to the library) or the default, clamped as
    the library clamps it"""
    n = 6
    for kv in os.environ.get("RAL_TEST_OPTIONS", "").split(","):
        if kv.strip() and kv.split("=")[0].strip().lower() in ("dw_sets", "ral_dw_sets"):
            n = int(kv.split("=")[1])
    return min(max(n, 2), 8)


# ---------------------------------------------------------------------------------------------------------------------
# GPU side
# ---------------------------------------------------------------------------------------------------------------------
def set_schedule(m, lanes, side):
    from ecg_denoise_amd import _lib
    _lib.check(_lib.lib().ral_set_option(m.eng.h, b"lanes", lanes))
    _lib.check(_lib.lib().ral_set_option(m.eng.h, b"side_stream", side))


def read_timeline(m, cap=4096):
    import ctypes as C
    from ecg_denoise_amd import _lib
    rows = (C.c_double * (4 * cap))()
    n = C.c_int64()
    _lib.check(_lib.lib().ral_profile_timeline(m.eng.h, rows, cap, C.byref(n)))
    return [(KINDS[int(rows[4 * i])], int(rows[4 * i + 1]), rows[4 * i + 2], rows[4 * i + 3]) for i in range(n.value)]


def train_pass(m, x, t, want_dx=False):
    """forward, loss, backward of one train step (no optimiser step: the parameters stay)"""
    y = m(x)
    loss, _, _ = m.loss_and_metrics(y, t)
    dx = m.backward(want_dx=want_dx)
    return y, loss, dx


def profiled_step(m, x, t):
    """one warm step with every kind selected (it creates the events), then the recorded one -> its rows"""
    import torch
    from ecg_denoise_amd import _lib
    lib, h = _lib.lib(), m.eng.h
    m.train()
    _lib.check(lib.ral_profile_select(h, b"*"))
    train_pass(m, x, t)
    torch.cuda.synchronize()
    _lib.check(lib.ral_profile_select(h, b"*"))
    train_pass(m, x, t)
    torch.cuda.synchronize()
    rows = read_timeline(m)
    _lib.check(lib.ral_profile_select(h, b""))
    return rows


def rwave_tables(m, seed):
    """R-wave tables of 0.3 * randn (the model's own initial tables are zero, which would hide the bias path)"""
    import torch
    g = torch.Generator().manual_seed(seed)
    for k, v in m.named_parameters():
        if "relative_position_bias_table" in k:
            v.copy_(0.3 * torch.randn(v.shape, generator=g))
    m._params_changed()


def main():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from ecg_denoise_amd import RALENet, _lib
    _lib.apply_options(os.environ.get("RAL_TEST_OPTIONS", ""))     # as tests/conftest.py does: expected_sets() reads the same variable
    B = int(sys.argv[1])
    m = RALENet("full", leads=1, L=256, max_batch=B, device="cuda:0", seed=3)
    rwave_tables(m, 4)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, 1, 256, generator=g).to("cuda:0"); t = torch.randn(B, 1, 256, generator=g).to("cuda:0")
    rows = profiled_step(m, x, t)
    chain = []
    for r in rows:
        if r[0] == "attn_fwd" and r[1] not in chain:
            chain.append(r[1])
    dw_on_chain = all(r[1] in chain for r in rows if r[0] == "dw")
    found, bad = check_timeline(rows, len(chain), 0 if dw_on_chain else 1, expected_sets())
    print("SCHEDULE " + json.dumps({"found": found, "violations": bad, "dw_on_chain": dw_on_chain}))


if __name__ == "__main__":
    main()
