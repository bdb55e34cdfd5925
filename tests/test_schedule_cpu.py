"""The timeline checker of tests/schedule_util.py on synthetic timelines: consistent ones pass, and each defect the GPU tests
rely on it to see is reported under its own name; the pure-Python helpers of tests/stall_util.py on synthetic inputs (no GPU)."""
import pytest
import torch

import schedule_util as S
import stall_util as ST

U = 1.0 / 1024      # ms; every stamp is a multiple of it (exact in binary floating point)


def synth(lanes, side, sets, ready_edge=True, done_edge=True, dw_len=9):
    """(kind, stream, t0, t1) rows of one train step as the library issues it: chain stream c = lane c, side stream lanes + c.
    A chain launch takes 2 U, a weight-gradient launch dw_len U (longer than its block's chain: with few sets the chain waits)."""
    rows, cur = [], [0.0] * (2 * lanes)

    def put(kind, s, dur, not_before=0.0):
        t0 = max(cur[s], not_before)
        cur[s] = t0 + dur * U
        rows.append((kind, s, t0, cur[s]))
        return rows[-1]

    for stage in range(9):
        for c in range(lanes):
            for _ in range(2):
                put("qkv_fwd", c, 2); put("attn_fwd", c, 2); put("mlp_fwd", c, 2)
        if stage != 4:
            for c in range(lanes):
                put("resample_fwd", c, 1)
    t_bwd = max(cur)
    dw_end = [[] for _ in range(lanes)]
    for stage in range(9):
        if stage != 4:
            for c in range(lanes):
                put("resample_bwd", c, 1, t_bwd)
        for c in range(lanes):
            for _ in range(2):
                j = len(dw_end[c])
                free = dw_end[c][j - sets] if (side and done_edge and j >= sets) else 0.0
                put("mlp_bwd", c, 2, max(free, t_bwd)); put("attn_bwd", c, 2)
                q = put("qkv_bwd", c, 2)
                d = put("dw", lanes + c if side else c, dw_len, q[3] if ready_edge else t_bwd)
                dw_end[c].append(d[3])
    return rows


@pytest.mark.parametrize("lanes,side,sets", [(4, 1, 2), (1, 0, 6), (2, 1, 6), (3, 0, 8), (1, 1, 2)])
def test_consistent_timeline_passes(lanes, side, sets):
    found, bad = S.check_timeline(synth(lanes, side, sets), lanes, side, sets)
    assert not bad, bad
    assert found["lanes"] == lanes and found["quantum_ms"] == U
    assert all(n == 18 * lanes for n in found["counts"].values())
    assert len(found["dw_streams"]) == lanes
    if side:
        assert found["edges_done"] == lanes * (18 - sets)
        if sets == 2:
            assert found["waits"] > 0 and found["slack_done_ms"] == 0.0     # the long dw makes the chain wait: the edge is used
        assert found["slack_ready_ms"] == 0.0


def test_kind_indices_are_accepted_like_names():
    rows = [(S.KINDS.index(k), s, a, b) for k, s, a, b in synth(2, 1, 2)]
    found, bad = S.check_timeline(rows, 2, 1, 2)
    assert not bad and found["lanes"] == 2


def test_dw_that_starts_before_its_qkv_bwd_ends_is_flagged():
    found, bad = S.check_timeline(synth(4, 1, 2, ready_edge=False), 4, 1, 2)
    assert S.EV_READY in S.names(bad), bad
    assert found["slack_ready_ms"] < -U


def test_one_early_dw_is_enough():
    rows = synth(4, 1, 2)
    i = next(i for i, r in enumerate(rows) if r[0] == "dw")        # the first dw of its side stream: nothing in front of it
    k, s, t0, t1 = rows[i]
    rows[i] = (k, s, t0 - 3 * U, t1)
    assert S.names(S.check_timeline(rows, 4, 1, 2)[1]) == [S.EV_READY]
    rows[i] = (k, s, t0 - U, t1)                                   # one quantum is allowed
    assert not S.check_timeline(rows, 4, 1, 2)[1]


def test_set_reused_before_its_dw_ended_is_flagged():
    found, bad = S.check_timeline(synth(4, 1, 2, done_edge=False), 4, 1, 2)
    assert S.names(bad) == [S.EV_DONE], bad
    assert found["slack_done_ms"] < -U
    # the same timeline is consistent for a schedule with 8 sets: the edge is only due 8 blocks later
    assert S.EV_DONE not in S.names(S.check_timeline(synth(4, 1, 8, done_edge=False, dw_len=3), 4, 1, 8)[1])


def test_one_lane_too_few_is_flagged():
    found, bad = S.check_timeline(synth(3, 1, 2), 4, 1, 2)
    assert S.LANES in S.names(bad), bad
    assert found["lanes"] == 3
    found, bad = S.check_timeline(synth(1, 0, 6), 2, 0, 6)         # a step that silently ran one lane
    assert S.LANES in S.names(bad) and found["lanes"] == 1


def test_dw_on_a_chain_stream_while_side_streams_are_expected_is_flagged():
    found, bad = S.check_timeline(synth(2, 0, 6), 2, 1, 6)
    assert S.names(bad) == [S.DW_STREAM], bad
    # and the other way round
    assert S.names(S.check_timeline(synth(2, 1, 6), 2, 0, 6)[1]) == [S.DW_STREAM]


def test_two_lanes_sharing_one_side_stream_are_flagged():
    rows = [(k, 2 if (k == "dw" and s == 3) else s, a, b) for k, s, a, b in synth(2, 1, 8, dw_len=1)]
    assert S.DW_STREAM in S.names(S.check_timeline(rows, 2, 1, 8)[1])


@pytest.mark.parametrize("kind", S.PER_BLOCK)
def test_launch_count_other_than_18_per_lane_is_flagged(kind):
    rows = synth(2, 1, 6)
    i = max(i for i, r in enumerate(rows) if r[0] == kind)
    del rows[i]
    found, bad = S.check_timeline(rows, 2, 1, 6)
    assert S.COUNT in S.names(bad), bad
    assert found["counts"][kind] == 35


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("kind", S.PER_BLOCK)
def test_a_kind_with_no_rows_at_all_is_flagged(kind, side):
    rows = [r for r in synth(2, side, 6) if r[0] != kind]
    found, bad = S.check_timeline(rows, 2, side, 6)
    assert S.COUNT in S.names(bad), bad
    assert found["counts"][kind] == 0


def test_invariants_must_have_run_over_every_block():
    found, bad = S.check_timeline(synth(2, 1, 6), 2, 1, 6)
    assert not bad and found["edges_ready"] == 36 and found["edges_done"] == 24
    rows = [r for r in synth(2, 1, 6) if r[0] != "dw"]
    found, bad = S.check_timeline(rows, 2, 1, 6)
    assert found["edges_ready"] == 0 and found["edges_done"] == 0 and found["slack_ready_ms"] is None
    assert {S.COUNT, S.DW_STREAM} <= set(S.names(bad))


def test_overlap_on_one_stream_is_flagged():
    rows = synth(1, 0, 6)
    k, s, t0, t1 = rows[10]
    rows[10] = (k, s, t0, t1 + 4 * U)
    assert S.names(S.check_timeline(rows, 1, 0, 6)[1]) == [S.OVERLAP]


def test_expected_sets_follows_the_test_options(monkeypatch):
    monkeypatch.delenv("RAL_TEST_OPTIONS", raising=False)
    assert S.expected_sets() == 6
    monkeypatch.setenv("RAL_TEST_OPTIONS", "attn_f16=0,dw_sets=2")
    assert S.expected_sets() == 2
    monkeypatch.setenv("RAL_TEST_OPTIONS", "dw_sets=11")
    assert S.expected_sets() == 8


# ---------------------------------------------------------------------------------------------------------------------
# tests/stall_util.py
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enqueue_ms,want", [(0.0, 20.0), (1.0, 20.0), (5.0, 20.0), (5.25, 21.0), (30.0, 120.0), (62.5, 250.0), (400.0, 250.0)])
def test_stall_is_four_times_the_enqueue_time_between_floor_and_cap(enqueue_ms, want):
    assert ST.stall_ms_for(enqueue_ms) == want


def test_broken_premise_fails_with_its_message():
    ST.check_premise(True, 20.0)
    for pending in (False, None, 1):
        with pytest.raises(AssertionError, match=r"premise failed \(case x\): the stall of 20.0 ms had ended"):
            ST.check_premise(pending, 20.0, "case x")


def test_stream_gaps_of_a_device_led_and_a_host_led_timeline():
    # device-led: launches back to back on stream 0; host-led: 1 U of work every 4 U on stream 1
    rows = [("qkv_fwd", 0, 2 * i * U, 2 * (i + 1) * U) for i in range(8)] + [("dw", 1, 4 * i * U, (4 * i + 1) * U) for i in range(5)]
    g = ST.stream_gaps(rows)
    assert g[0] == {"rows": 8, "busy": 1.0, "median_gap_ms": 0.0, "max_gap_ms": 0.0}
    assert g[1]["rows"] == 5 and g[1]["busy"] == 5.0 / 17.0 and g[1]["median_gap_ms"] == 3 * U and g[1]["max_gap_ms"] == 3 * U
    assert ST.least_busy(rows, [0]) == 1.0 and ST.least_busy(rows, [0, 1]) == 5.0 / 17.0
    assert ST.least_busy(rows, [7]) == 1.0                          # a stream without rows
    # issue order, not time order, pairs the rows; an overlap counts as no gap; an even number of gaps takes the middle pair
    rows = [("dw", 3, 0.0, 4 * U), ("dw", 3, 3 * U, 5 * U), ("dw", 3, 7 * U, 8 * U)]
    g = ST.stream_gaps(rows)[3]
    assert g["median_gap_ms"] == U and g["max_gap_ms"] == 2 * U and g["busy"] == 7.0 / 8.0
    assert ST.stream_gaps([("dw", 0, 1.0, 1.0)])[0]["busy"] == 1.0   # a single stamp
    assert ST.stream_gaps([]) == {}


def test_stream_gaps_of_the_synthetic_step():
    rows = synth(2, 1, 2)
    g = ST.stream_gaps(rows)
    assert sorted(g) == [0, 1, 2, 3] and [g[s]["rows"] for s in (2, 3)] == [18, 18]
    assert g[2]["busy"] == 1.0 and g[2]["max_gap_ms"] == 0.0         # the long dw keeps the side stream busy: the chain waits
    assert ST.least_busy(rows, [0, 1]) < 1.0


def test_poison_and_late_on_host_tensors():
    f, i, u = torch.ones(3), torch.ones(3, dtype=torch.int32), torch.ones(3, dtype=torch.uint8)
    assert torch.isnan(ST.poison(f)).all()
    assert (ST.poison(i) == -12345).all() and (ST.poison(u) == 123).all()
    assert torch.equal(ST.late(f, torch.arange(3.0)), torch.arange(3.0))
