"""RA-LENet pass (csrc/ral_ralenet_plan.*) on the CPU, through `ral_ralenet_node_geom` / `ral_ralenet_pass_plan` alone: the node
table against a copy written out here, the state-dict prefixes of the layout, the forward and backward passes against the
launch sites the model had before the table existed (copied here by hand as tuples), the issue order under 1 .. 4 lanes, the
bucket mark, the lane split and every refusal."""
import ctypes as C

import pytest

from ecg_denoise_amd import _lib

# tensor ids
X0 = 0
S = list(range(1, 10))                    # outputs of stages 0 .. 8 (the old act[2 si + 1].out)
P1, P2, P3, P4, XMID, U3, U2, U1, U0 = range(10, 19)
# gradient buffer ids, under the names the workspace registers
GY = list(range(18))
GIN = list(range(18, 27))
DU0 = 27
NONE = -1

# kind index level rw D up | in addend out
TABLE = [
    (0, 0, 0, 1, 0, 0, X0, NONE, S[0]),     (1, 0, 1, 0, 16, 0, S[0], NONE, P1),
    (0, 1, 1, 2, 0, 0, P1, NONE, S[1]),     (1, 1, 2, 0, 32, 0, S[1], NONE, P2),
    (0, 2, 2, 3, 0, 0, P2, NONE, S[2]),     (1, 2, 3, 0, 64, 0, S[2], NONE, P3),
    (0, 3, 3, 4, 0, 0, P3, NONE, S[3]),     (1, 3, 4, 0, 128, 0, S[3], NONE, P4),
    (0, 4, 4, 0, 0, 0, P4, P4, XMID),
    (0, 5, 4, 0, 0, 0, XMID, NONE, S[5]),   (1, 4, 3, 0, 64, 1, S[5], P3, U3),
    (0, 6, 3, 4, 0, 0, U3, NONE, S[6]),     (1, 5, 2, 0, 32, 1, S[6], P2, U2),
    (0, 7, 2, 3, 0, 0, U2, NONE, S[7]),     (1, 6, 1, 0, 16, 1, S[7], P1, U1),
    (0, 8, 1, 2, 0, 0, U1, NONE, S[8]),     (1, 7, 0, 0, 8, 1, S[8], NONE, U0),
]
NAMES = ["dtransformer1", "pm1", "dtransformer2", "pm2", "dtransformer3", "pm3", "dtransformer34", "pm4", "transformer",
         "utransformer4", "ps4", "utranformer3", "ps3", "utransformer2", "ps2", "utransformer1", "ps1"]
STAGE_NODE = [0, 2, 4, 6, 8, 9, 11, 13, 15]
RES_NODE = [1, 3, 5, 7, 10, 12, 14, 16]

# The backward as the model issued it before the table: (node, dy, extra, dx, forward input read again).  A run_res_bwd(m, ri,
# dy, act[b].out, dx) line gives (RES_NODE[ri], dy, none, dx, S[b // 2]); a run_stage_bwd(m, si, dy, extra, tmp, dx) line gives
# (STAGE_NODE[si], dy, extra, dx, the stage's forward input), its tmp is gy[2 si].
BACKWARD = [
    (16, DU0, NONE, GY[17], S[8]),          # run_res_bwd(7, du0, act[17].out, gy[17])
    (15, GY[17], NONE, GIN[8], U1),         # run_stage_bwd(8, gy[17], nullptr, gy[16], gin[8])          g u1
    (14, GIN[8], NONE, GY[15], S[7]),       # run_res_bwd(6, gin[8], act[15].out, gy[15])
    (13, GY[15], NONE, GIN[7], U2),         # run_stage_bwd(7, gy[15], nullptr, gy[14], gin[7])          g u2
    (12, GIN[7], NONE, GY[13], S[6]),       # run_res_bwd(5, gin[7], act[13].out, gy[13])
    (11, GY[13], NONE, GIN[6], U3),         # run_stage_bwd(6, gy[13], nullptr, gy[12], gin[6])          g u3
    (10, GIN[6], NONE, GY[11], S[5]),       # run_res_bwd(4, gin[6], act[11].out, gy[11])
    (9, GY[11], NONE, GIN[5], XMID),        # run_stage_bwd(5, gy[11], nullptr, gy[10], gin[5])          g x_mid; the bucket mark follows
    (8, GIN[5], GIN[5], GIN[4], P4),        # run_stage_bwd(4, gin[5], gin[5], gy[8], gin[4])            gy[9] = gin[5]
    (7, GIN[4], NONE, GY[7], S[3]),         # run_res_bwd(3, gin[4], act[7].out, gy[7])
    (6, GY[7], GIN[6], GIN[3], P3),         # run_stage_bwd(3, gy[7], gin[6], gy[6], gin[3])             g p3 (+ g u3)
    (5, GIN[3], NONE, GY[5], S[2]),         # run_res_bwd(2, gin[3], act[5].out, gy[5])
    (4, GY[5], GIN[7], GIN[2], P2),         # run_stage_bwd(2, gy[5], gin[7], gy[4], gin[2])             g p2 (+ g u2)
    (3, GIN[2], NONE, GY[3], S[1]),         # run_res_bwd(1, gin[2], act[3].out, gy[3])
    (2, GY[3], GIN[8], GIN[1], P1),         # run_stage_bwd(1, gy[3], gin[8], gy[2], gin[1])             g p1 (+ g u1)
    (1, GIN[1], NONE, GY[1], S[0]),         # run_res_bwd(0, gin[1], act[1].out, gy[1])
    (0, GY[1], DU0, GIN[0], X0),            # run_stage_bwd(0, gy[1], du0, gy[0], gin[0])                g x0 (+ d u0)
]
MARK_AFTER_NODE = 9                       # after stage 5, utransformer4: the decoder's last backward node
# The forward: (node, input, addend, output): stages 0 .. 3 from x0 / p_k, the bottleneck p4 -> xmid with p4 added, stages 5 .. 8
# from xmid / u_k; run_res_fwd(4 + i, act[2 (5 + i) + 1].out, i < 3 ? res_out[2 - i] : nullptr) = the skips p3, p2, p1, none
FORWARD = [(i,) + TABLE[i][6:9] for i in range(17)]
FORWARD_SKIPS = {10: P3, 12: P2, 14: P1, 16: NONE}


def lib():
    return _lib.lib()


def node(i):
    row = (C.c_int32 * 9)()
    assert lib().ral_ralenet_node_geom(i, row, 9) == 17, lib().ral_last_error()
    return tuple(row)


def entries(backward, B, lanes):
    row = (C.c_int32 * 9)()
    n = lib().ral_ralenet_pass_plan(backward, B, lanes, 0, row, 9)
    assert n > 0, lib().ral_last_error()
    out = []
    for k in range(n):
        assert lib().ral_ralenet_pass_plan(backward, B, lanes, k, row, 9) == n, lib().ral_last_error()
        out.append(tuple(row))
    return out


def test_node_table_equals_the_copy_written_out_here():
    assert [node(i) for i in range(17)] == TABLE
    assert [i for i in range(17) if TABLE[i][0] == 0] == STAGE_NODE and [TABLE[i][1] for i in STAGE_NODE] == list(range(9))
    assert [i for i in range(17) if TABLE[i][0] == 1] == RES_NODE and [TABLE[i][1] for i in RES_NODE] == list(range(8))
    for r in TABLE:
        if r[0] == 1:
            assert r[4] == 8 << r[2]          # a resampler's width is the width of its output's level


@pytest.mark.parametrize("variant", ["nra", "full", "mlp"])
def test_state_dict_prefixes_of_the_layout_follow_the_table(variant):
    """the layout walks the table: between the stem / R-wave tables and transconv, the distinct first name components, in order,
    are the 17 node names (with the reference's spelling utranformer3)"""
    ent = _lib.layout(_lib.make_config(variant, 1, 256, 4, 1))
    seen = []
    for e in ent:
        p = e["name"].split(".")[0]
        if p not in seen:
            seen.append(p)
    body = [p for p in seen if p not in ("conv1", "transconv") and not p.startswith("rwattn")]
    assert body == NAMES
    assert seen[0] == "conv1" and seen[-1] == "transconv"


def test_backward_pass_equals_the_eighteen_launch_sites():
    got = entries(1, 4, 1)
    assert [(e[0], e[4], e[5], e[6], e[7]) for e in got] == BACKWARD
    assert all(e[1:4] == (0, 0, 4) for e in got)
    # the rule the extras follow: the gradient of the output of the node that takes this stage's input tensor as its addend
    dy_of = {TABLE[n][8]: dy for n, dy, _, _, _ in BACKWARD}                    # output tensor -> its gradient buffer
    for n, dy, extra, dx, fin in BACKWARD:
        assert fin == TABLE[n][6]
        if TABLE[n][0] == 1:
            assert extra == NONE
            continue
        takers = [t for t in TABLE if t[7] == fin]
        if fin == X0:                                                           # the head computes u0 + x0
            assert not takers and extra == DU0
        else:
            assert extra == (dy_of[takers[0][8]] if takers else NONE)
    # the bottleneck's output gradient is the gradient of xmid, gin5: no entry names gy9
    assert BACKWARD[8][1] == GIN[5] and all(GY[9] not in e[4:7] for e in got)
    # gin<s> is the gradient of stage s's input; a node's dx is the dy of the node that produced its input
    for n, dy, _, dx, fin in BACKWARD:
        if TABLE[n][0] == 0:
            assert dx == GIN[TABLE[n][1]]
        if n > 0:
            assert dx == BACKWARD[16 - (n - 1)][1]


def test_forward_pass_equals_the_launch_sites():
    got = entries(0, 4, 1)
    assert [(e[0], e[4], e[5], e[6]) for e in got] == FORWARD
    assert all(e[7] == NONE and e[8] == 0 and e[1:4] == (0, 0, 4) for e in got)
    assert {n: got[n][5] for n in FORWARD_SKIPS} == FORWARD_SKIPS
    assert got[8][4:7] == (P4, P4, XMID) and got[9][4] == XMID
    assert [got[n][5] for n in STAGE_NODE if n != 8] == [NONE] * 8
    for a, b in zip(got, got[1:]):                                              # every node reads what the node before it wrote
        assert b[4] == a[6]


@pytest.mark.parametrize("lanes", [1, 2, 3, 4])
@pytest.mark.parametrize("backward", [0, 1])
def test_issue_order_node_by_node_every_lane_of_a_node_first(backward, lanes):
    B = 64 * lanes
    got = entries(backward, B, lanes)
    one = entries(backward, B, 1)
    assert len(got) == 17 * lanes and len(one) == 17
    for k, e in enumerate(got):
        ref = one[k // lanes]
        assert e[0] == ref[0] and e[4:8] == ref[4:8]
        assert e[1:4] == (k % lanes, 64 * (k % lanes), 64)


@pytest.mark.parametrize("lanes", [1, 2, 3, 4])
def test_bucket_mark_follows_the_last_lane_of_stage_five(lanes):
    got = entries(1, 64 * lanes, lanes)
    marks = [k for k, e in enumerate(got) if e[8]]
    assert marks == [8 * lanes - 1]
    assert got[marks[0]][0] == MARK_AFTER_NODE and got[marks[0]][1] == lanes - 1 and got[marks[0] + 1][0] == 8
    assert NAMES[MARK_AFTER_NODE] == "utransformer4"
    assert not any(e[8] for e in entries(0, 64 * lanes, lanes))


@pytest.mark.parametrize("lanes,B,expect", [(3, 192, 3), (3, 190, 1), (3, 189, 1), (3, 64, 1), (4, 255, 1), (2, 128, 2), (2, 127, 1),
                                            (4, 256, 4), (1, 1, 1), (1, 63, 1), (1, 64, 1), (1, 4096, 1)])
def test_lane_split(lanes, B, expect):
    for backward in (0, 1):
        got = entries(backward, B, lanes)
        assert len(got) == 17 * expect
        assert [e[1:4] for e in got[:expect]] == [(k, k * (B // expect), B // expect) for k in range(expect)]
    if (lanes, B) == (4, 256):
        assert [e[2] for e in got[:4]] == [0, 64, 128, 192]


def test_refusals():
    L = lib()
    row = (C.c_int32 * 9)()
    for args, text in [((-1, row, 9), b"RA-LENet node -1 outside [0, 16]"), ((17, row, 9), b"RA-LENet node 17 outside [0, 16]"),
                       ((0, row, 8), b"RA-LENet node row: room for 9 values is needed (got 8)"),
                       ((0, None, 9), b"RA-LENet node row: room for 9 values is needed (got 0)")]:
        assert L.ral_ralenet_node_geom(*args) < 0 and L.ral_last_error() == text
    for args, text in [((0, 0, 1, 0, row, 9), b"RA-LENet pass: B must be positive (got 0)"),
                       ((0, 4, 0, 0, row, 9), b"RA-LENet pass: lanes must be in [1, 4] (got 0)"),
                       ((1, 4, 5, 0, row, 9), b"RA-LENet pass: lanes must be in [1, 4] (got 5)"),
                       ((1, 4, 1, -1, row, 9), b"RA-LENet pass: entry -1 outside [0, 17)"),
                       ((0, 4, 1, 17, row, 9), b"RA-LENet pass: entry 17 outside [0, 17)"),
                       ((0, 128, 2, 34, row, 9), b"RA-LENet pass: entry 34 outside [0, 34)"),
                       ((0, 127, 2, 17, row, 9), b"RA-LENet pass: entry 17 outside [0, 17)"),
                       ((0, 4, 1, 0, row, 8), b"RA-LENet pass row: room for 9 values is needed (got 8)"),
                       ((0, 4, 1, 0, None, 9), b"RA-LENet pass row: room for 9 values is needed (got 0)")]:
        assert L.ral_ralenet_pass_plan(*args) < 0 and L.ral_last_error() == text
