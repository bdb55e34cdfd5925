"""Baseline network dispatch (csrc/ral_baseline_plan.*) on the CPU, through `ral_baseline_layer_geom` / `ral_baseline_pass_plan`
alone: the two tables and the kernel instance lists against copies written out here, launch numbers worked out by hand from the
formulas the launch sites of ral_acdae.hip / ral_danet.hip had before the plan existed, a sweep of the whole legal space for what
every launch must satisfy, the refusals, and the ledger: the cases of the oracle and golden GPU tests of the two networks, read
from those tests' own parametrize marks, launch every one of the 13 + 18 kernel instances."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ecg_denoise_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACDAE, DANET = 4, 5                      # RAL_ACDAE, RAL_DANET
BATCHES = (1, 3, 511, 512, 513, 1024, 1025, 2048, 4096)
ACDAE_LS, DANET_LS = range(64, 1025, 64), range(32, 2049, 16)      # the legal window lengths
LDS_MAX = 160 * 1024

ACDAE_INSTANCES = ["k_acd_enc_fwd<13>", "k_acd_enc_fwd<7>", "k_acd_enc_fwd_m<7>", "k_acd_dec_fwd<7>", "k_acd_dec_fwd<13>", "k_acd_dec_bwd<7>",
                   "k_acd_dec_bwd<13>", "k_acd_enc_bwd<13>", "k_acd_enc_bwd<7>", "k_acd_dw_m<13, false>", "k_acd_dw_m<7, false>", "k_acd_dw_m<7, true>",
                   "k_acd_dw<13, true>"]
DANET_INSTANCES = (["k_dn_conv%s<%s>" % (b, a) for b in ("", "_b") for a in ("17, false", "3, false", "4, true", "18, true")]
                   + ["k_dn_fcn_mid", "k_dn_act<4>", "k_dn_act<1>", "k_dn_dam1", "k_dn_out", "k_dn_dam_b", "k_dn_fcn_bmid", "k_dn_bn_b", "k_dn_act_b<4>",
                      "k_dn_act_b<1>"])
# weight-gradient instances that were built before the plan and that no row can reach: the MFMA form takes every row with 16 or more
# output channels (all but decoder 3, 13 taps, transposed), the scalar form only that one
NO_LONGER_BUILT = ["k_acd_dw<13, false>", "k_acd_dw<7, false>", "k_acd_dw<7, true>", "k_acd_dw_m<13, true>"]

# ---- the tables.  ACDAE: cin cout ks convt in_shift out_shift skip (rows 0-3 encoder, 4-7 decoder; lengths L >> shift)
ACDAE_ROWS = [(2, 16, 13, 0, 0, 1, -1), (16, 32, 7, 0, 1, 2, -1), (32, 64, 7, 0, 2, 3, -1), (64, 128, 7, 0, 3, 4, -1),
              (128, 64, 7, 1, 4, 3, 2), (64, 32, 7, 1, 3, 2, 1), (32, 16, 7, 1, 2, 1, 0), (16, 2, 13, 1, 1, 0, -1)]
# DANet: cin c k p tr in_shift out_shift in1 dam (rows 0-3 encoder cells, 4-7 decoder cells)
DANET_ROWS = [(2, 4, 17, 8, 0, 0, 1, -1, 0), (4, 8, 17, 8, 0, 1, 2, -1, 0), (8, 16, 3, 1, 0, 2, 3, -1, 0), (16, 32, 3, 1, 0, 3, 4, -1, 0),
              (32, 16, 4, 1, 1, 4, 3, -1, 1), (16, 8, 4, 1, 1, 3, 2, 2, 1), (8, 4, 18, 8, 1, 2, 1, 1, 1), (4, 2, 18, 8, 1, 1, 0, 0, 0)]

# ---- launch numbers, by hand from the launch sites of the parent commit.  ACDAE entries: (kernel, grid x, grid y, LDS bytes, NG);
# every kernel has 256 threads.  lin: the row's input length; grid = min(B, 1024) unless said otherwise.
#   k_acd_enc_fwd     4 cin (lin + 16)                            e.g. (512, 2048) encoder 0: 4 * 2 * 528 = 4224
#   k_acd_enc_fwd_m   that + 4 * 32 cin 7; grid (min(B, 512), cout / 32)     encoder 1: 4 * 16 * 272 + 128 * 16 * 7 = 31744, grid (512, 1)
#   k_acd_dec_fwd     4 (cin (lin + 16) + 3 cout lin + 2 cout + 8)           decoder 0: 4 * (128 * 48 + 3 * 64 * 32 + 136) = 49696
#   k_acd_dec_bwd     4 (2 cout lin + cout (lin + 16) + 3 cout + 16)         decoder 0: 4 * (4096 + 3072 + 208) = 29504
#   k_acd_enc_bwd     4 cout (lin + 16)                                      encoder 3: 4 * 128 * 80 = 40960
#   k_acd_dw_m        cout >= 16: MT = ceil(cout / 16), NT = ceil(cin ks / 16), NG = ceil(NT / 16); grid (MT NG, min(max(512 // (MT NG), 1), B));
#                     cxr = min(256 // ks + 2, cin); 4 (16 lin + cxr (lin + 16))
#                     decoder 0 (cout 64, cin 128, lin 32): MT 4, NT 56, NG 4: grid (16, 32); cxr 38: 4 * (512 + 38 * 48) = 9344
#   k_acd_dw          nblk = ceil(cout / 8) ceil(cin / 8); grid (nblk, min(max(2048 // nblk, 1), B)); 4 (8 lin + 8 (lin + 16))
#                     decoder 3 (cout 2, cin 16, lin 256): nblk 2: grid (2, 1024); 4 * (2048 + 2176) = 16896
ACDAE_LAUNCHES = {
    (512, 2048, 'fwd'): [
        ('k_acd_enc_fwd<13>', 1024, 1, 4224, 0), ('k_acd_enc_fwd_m<7>', 512, 1, 31744, 0),
        ('k_acd_enc_fwd_m<7>', 512, 2, 47104, 0), ('k_acd_enc_fwd_m<7>', 512, 4, 77824, 0),
        ('k_acd_dec_fwd<7>', 1024, 1, 49696, 0), ('k_acd_dec_fwd<7>', 1024, 1, 45344, 0),
        ('k_acd_dec_fwd<7>', 1024, 1, 43168, 0), ('k_acd_dec_fwd<13>', 1024, 1, 23600, 0),
    ],
    (512, 2048, 'bwd'): [
        ('k_acd_dec_bwd<13>', 1024, 1, 6360, 0), ('k_acd_dw<13, true>', 2, 1024, 16896, 0),
        ('k_acd_dec_bwd<7>', 1024, 1, 25856, 0), ('k_acd_dw_m<7, true>', 1, 512, 26624, 1),
        ('k_acd_dec_bwd<7>', 1024, 1, 27072, 0), ('k_acd_dw_m<7, true>', 4, 128, 16256, 2),
        ('k_acd_dec_bwd<7>', 1024, 1, 29504, 0), ('k_acd_dw_m<7, true>', 16, 32, 9344, 4),
        ('k_acd_enc_bwd<7>', 1024, 1, 40960, 0), ('k_acd_dw_m<7, false>', 16, 32, 16256, 2),
        ('k_acd_enc_bwd<7>', 1024, 1, 36864, 0), ('k_acd_dw_m<7, false>', 4, 128, 26624, 1),
        ('k_acd_enc_bwd<7>', 1024, 1, 34816, 0), ('k_acd_dw_m<7, false>', 2, 256, 33792, 1),
        ('k_acd_enc_bwd<13>', 1024, 1, 33792, 0), ('k_acd_dw_m<13, false>', 1, 512, 36992, 1),
    ],
    (1024, 2, 'fwd'): [
        ('k_acd_enc_fwd<13>', 2, 1, 8320, 0), ('k_acd_enc_fwd_m<7>', 2, 1, 48128, 0),
        ('k_acd_enc_fwd_m<7>', 2, 2, 63488, 0), ('k_acd_enc_fwd_m<7>', 2, 4, 94208, 0),
        ('k_acd_dec_fwd<7>', 2, 1, 90656, 0), ('k_acd_dec_fwd<7>', 2, 1, 86304, 0),
        ('k_acd_dec_fwd<7>', 2, 1, 84128, 0), ('k_acd_dec_fwd<13>', 2, 1, 46128, 0),
    ],
    (1024, 2, 'bwd'): [
        ('k_acd_dec_bwd<13>', 2, 1, 12504, 0), ('k_acd_dw<13, true>', 2, 2, 33280, 0),
        ('k_acd_dec_bwd<7>', 2, 1, 50432, 0), ('k_acd_dw_m<7, true>', 1, 2, 51200, 1),
        ('k_acd_dec_bwd<7>', 2, 1, 51648, 0), ('k_acd_dw_m<7, true>', 4, 2, 30080, 2),
        ('k_acd_dec_bwd<7>', 2, 1, 54080, 0), ('k_acd_dw_m<7, true>', 16, 2, 16256, 4),
        ('k_acd_enc_bwd<7>', 2, 1, 73728, 0), ('k_acd_dw_m<7, false>', 16, 2, 30080, 2),
        ('k_acd_enc_bwd<7>', 2, 1, 69632, 0), ('k_acd_dw_m<7, false>', 4, 2, 51200, 1),
        ('k_acd_enc_bwd<7>', 2, 1, 67584, 0), ('k_acd_dw_m<7, false>', 2, 2, 66560, 1),
        ('k_acd_enc_bwd<13>', 2, 1, 66560, 0), ('k_acd_dw_m<13, false>', 1, 2, 73856, 1),
    ],
    (64, 3, 'fwd'): [
        ('k_acd_enc_fwd<13>', 3, 1, 640, 0), ('k_acd_enc_fwd_m<7>', 3, 1, 17408, 0),
        ('k_acd_enc_fwd_m<7>', 3, 2, 32768, 0), ('k_acd_enc_fwd<7>', 3, 1, 6144, 0),
        ('k_acd_dec_fwd<7>', 3, 1, 13856, 0), ('k_acd_dec_fwd<7>', 3, 1, 9504, 0),
        ('k_acd_dec_fwd<7>', 3, 1, 7328, 0), ('k_acd_dec_fwd<13>', 3, 1, 3888, 0),
    ],
    (64, 3, 'bwd'): [
        ('k_acd_dec_bwd<13>', 3, 1, 984, 0), ('k_acd_dw<13, true>', 2, 3, 2560, 0),
        ('k_acd_dec_bwd<7>', 3, 1, 4352, 0), ('k_acd_dw_m<7, true>', 1, 3, 5120, 1),
        ('k_acd_dec_bwd<7>', 3, 1, 5568, 0), ('k_acd_dw_m<7, true>', 4, 3, 4160, 2),
        ('k_acd_dec_bwd<7>', 3, 1, 8000, 0), ('k_acd_dw_m<7, true>', 16, 3, 3296, 4),
        ('k_acd_enc_bwd<7>', 3, 1, 12288, 0), ('k_acd_dw_m<7, false>', 16, 3, 4160, 2),
        ('k_acd_enc_bwd<7>', 3, 1, 8192, 0), ('k_acd_dw_m<7, false>', 4, 3, 5120, 1),
        ('k_acd_enc_bwd<7>', 3, 1, 6144, 0), ('k_acd_dw_m<7, false>', 2, 3, 5120, 1),
        ('k_acd_enc_bwd<13>', 3, 1, 5120, 0), ('k_acd_dw_m<13, false>', 1, 3, 4736, 1),
    ],
    (192, 2, 'fwd'): [
        ('k_acd_enc_fwd<13>', 2, 1, 1664, 0), ('k_acd_enc_fwd_m<7>', 2, 1, 21504, 0),
        ('k_acd_enc_fwd_m<7>', 2, 2, 36864, 0), ('k_acd_enc_fwd<7>', 2, 1, 10240, 0),
        ('k_acd_dec_fwd<7>', 2, 1, 24096, 0), ('k_acd_dec_fwd<7>', 2, 1, 19744, 0),
        ('k_acd_dec_fwd<7>', 2, 1, 17568, 0), ('k_acd_dec_fwd<13>', 2, 1, 9520, 0),
    ],
    (192, 2, 'bwd'): [
        ('k_acd_dec_bwd<13>', 2, 1, 2520, 0), ('k_acd_dw<13, true>', 2, 2, 6656, 0),
        ('k_acd_dec_bwd<7>', 2, 1, 10496, 0), ('k_acd_dw_m<7, true>', 1, 2, 11264, 1),
        ('k_acd_dec_bwd<7>', 2, 1, 11712, 0), ('k_acd_dw_m<7, true>', 4, 2, 7616, 2),
        ('k_acd_dec_bwd<7>', 2, 1, 14144, 0), ('k_acd_dw_m<7, true>', 16, 2, 5024, 4),
        ('k_acd_enc_bwd<7>', 2, 1, 20480, 0), ('k_acd_dw_m<7, false>', 16, 2, 7616, 2),
        ('k_acd_enc_bwd<7>', 2, 1, 16384, 0), ('k_acd_dw_m<7, false>', 4, 2, 11264, 1),
        ('k_acd_enc_bwd<7>', 2, 1, 14336, 0), ('k_acd_dw_m<7, false>', 2, 2, 13312, 1),
        ('k_acd_enc_bwd<13>', 2, 1, 13312, 0), ('k_acd_dw_m<13, false>', 1, 2, 13952, 1),
    ],
}

# DANet: every kernel has 256 threads and grid y = 1; the four grids are min(B, 1024) (conv, dam1, out, conv_b), min(ceil(B / 16), 256)
# (fcn_mid, fcn_bmid), min(ceil(B / 4), 256) (act, act_b) and min(B, 512) (dam_b, bn_b).  LDS bytes per cell and family, C = c:
#   conv    4 (cin (lin + 24) + c lout + 2 c)       e.g. L = 512 cell 0: 4 * (2 * 536 + 4 * 256 + 8) = 8416
#   dam1    4 c lout                                 cell 4: 4 * 16 * 64 = 4096        out 4 (c lout + lout): cell 0: 4 * (1024 + 256) = 5120
#   dam_b   4 (2 c lout + 3 lout)                    cell 4: 4 * (2048 + 192) = 8960
#   fcn_bmid  the DAM's fcn 4 (C C + C): cell 4: 4 * 272 = 1088; the APReLU's 4 (2 C C + C): cell 3: 4 * 2080 = 8320
#   bn_b    4 (c lout + [dam] (C C + C))             cell 4: 4096 + 1088 = 5184
#   conv_b  4 (cin (lin + 24) + c (lout + 24) + c cin k + c + 4 C C + 2 C)     cell 0: 4 * (1072 + 1120 + 136 + 4 + 64 + 8) = 9616
# v1: the cells whose output length is no multiple of 4 (k_dn_act<1> / k_dn_act_b<1>)
DANET_LDS = {
    (512, 2048): dict(grids=(1024, 128, 256, 512),
        conv=[8416, 8640, 9088, 9984, 11392, 9792, 8992, 8592], dam1=[None, None, None, None, 4096, 4096, 4096, None], out=[5120, 4608, 4352, 4224, 4352, 4608, 5120, 6144],
        dam_b=[None, None, None, None, 8960, 9728, 11264, None], bmid_dam=[None, None, None, None, 1088, 288, 80, None], bn_b=[4096, 4096, 4096, 4096, 5184, 4384, 4176, 4096],
        bmid_act=[144, 544, 2112, 8320, 2112, 544, 144, 40], conv_b=[9616, 12640, 16320, 35712, 25280, 13664, 11952, 9432],
        v1=[]),
    (32, 8): dict(grids=(8, 1, 2, 8),
        conv=[736, 960, 1408, 2304, 3712, 2112, 1312, 912], dam1=[None, None, None, None, 256, 256, 256, None], out=[320, 288, 272, 264, 272, 288, 320, 384],
        dam_b=[None, None, None, None, 560, 608, 704, None], bmid_dam=[None, None, None, None, 1088, 288, 80, None], bn_b=[256, 256, 256, 256, 1344, 544, 336, 256],
        bmid_act=[144, 544, 2112, 8320, 2112, 544, 144, 40], conv_b=[1936, 4960, 8640, 28032, 17600, 5984, 4272, 1752],
        v1=[3]),
    (64, 4): dict(grids=(4, 1, 1, 4),
        conv=[1248, 1472, 1920, 2816, 4224, 2624, 1824, 1424], dam1=[None, None, None, None, 512, 512, 512, None], out=[640, 576, 544, 528, 544, 576, 640, 768],
        dam_b=[None, None, None, None, 1120, 1216, 1408, None], bmid_dam=[None, None, None, None, 1088, 288, 80, None], bn_b=[512, 512, 512, 512, 1600, 800, 592, 512],
        bmid_act=[144, 544, 2112, 8320, 2112, 544, 144, 40], conv_b=[2448, 5472, 9152, 28544, 18112, 6496, 4784, 2264],
        v1=[]),
    (2048, 2): dict(grids=(2, 1, 1, 2),
        conv=[32992, 33216, 33664, 34560, 35968, 34368, 33568, 33168], dam1=[None, None, None, None, 16384, 16384, 16384, None], out=[20480, 18432, 17408, 16896, 17408, 18432, 20480, 24576],
        dam_b=[None, None, None, None, 35840, 38912, 45056, None], bmid_dam=[None, None, None, None, 1088, 288, 80, None], bn_b=[16384, 16384, 16384, 16384, 17472, 16672, 16464, 16384],
        bmid_act=[144, 544, 2112, 8320, 2112, 544, 144, 40], conv_b=[34192, 37216, 40896, 60288, 49856, 38240, 36528, 34008],
        v1=[]),
}


def danet_expected(L, B, backward):
    """[(cell, kernel, grid x, LDS bytes, extra)] of a pass, from the numbers above and the cell order of the launch sites; extra is
    the np argument of the two fcn kernels: 1 for the APReLU's fcn of a cell, 2 (both pooled paths) for the DAM's"""
    t = DANET_LDS[(L, B)]
    grid, gridd, grida, gridw = t["grids"]
    out = []
    for i in (range(7, -1, -1) if backward else range(8)):
        cin, c, k, p, tr, ish, osh, in1, dam = DANET_ROWS[i]
        conv = "<%d, %s>" % (k, "true" if tr else "false")
        v = 1 if i in t["v1"] else 4
        if not backward:
            out += [(i, "k_dn_conv" + conv, grid, t["conv"][i], 0), (i, "k_dn_fcn_mid", gridd, 0, 1), (i, "k_dn_act<%d>" % v, grida, 0, 0)]
            if dam:
                out += [(i, "k_dn_dam1", grid, t["dam1"][i], 0), (i, "k_dn_fcn_mid", gridd, 0, 2)]
            out += [(i, "k_dn_out", grid, t["out"][i], 0)]
        else:
            if dam:
                out += [(i, "k_dn_dam_b", gridw, t["dam_b"][i], 0), (i, "k_dn_fcn_bmid", gridd, t["bmid_dam"][i], 2)]
            out += [(i, "k_dn_bn_b", gridw, t["bn_b"][i], 0), (i, "k_dn_act_b<%d>" % v, grida, 0, 0), (i, "k_dn_fcn_bmid", gridd, t["bmid_act"][i], 1),
                    (i, "k_dn_conv_b" + conv, grid, t["conv_b"][i], 0)]
    return out


def passplan(variant, L, B, backward, training=1, lib=None):
    """[(layer, kernel name, grid x, grid y, threads, LDS bytes, extra)] of a pass; extra: NG of k_acd_dw_m, np of DANet's fcn kernels"""
    lib = lib or _lib.lib()
    n = lib.ral_baseline_pass_plan(variant, 2, L, B, training, backward, -1, None, 0, None, None, None, None, None, None)
    assert n > 0, lib.ral_last_error()
    name = C.create_string_buffer(64)
    layer, gx, gy, th, ng = (C.c_int32() for _ in range(5))
    lds = C.c_int64()
    out = []
    for k in range(n):
        rc = lib.ral_baseline_pass_plan(variant, 2, L, B, training, backward, k, name, len(name), C.byref(layer), C.byref(gx), C.byref(gy), C.byref(th),
                                        C.byref(lds), C.byref(ng))
        assert rc == 0, lib.ral_last_error()
        out.append((layer.value, name.value.decode(), gx.value, gy.value, th.value, lds.value, ng.value))
    return out


def test_the_instance_lists_are_the_13_and_18_of_the_header():
    hpp = open(os.path.join(ROOT, "ecg_denoise_amd", "csrc", "ral_baseline_plan.hpp")).read()
    listed = re.findall(r'^\s*X\(\w+, "([^"]+)"\)', hpp, flags=re.M)
    assert len(ACDAE_INSTANCES) == 13 and len(DANET_INSTANCES) == 18
    assert listed == ACDAE_INSTANCES + DANET_INSTANCES
    assert not set(NO_LONGER_BUILT) & set(listed)


@pytest.mark.parametrize("variant,rows", [(ACDAE, ACDAE_ROWS), (DANET, DANET_ROWS)], ids=["acdae", "danet"])
def test_layer_tables(variant, rows):
    lib = _lib.lib()
    n = len(rows[0])
    row = (C.c_int32 * n)()
    got = []
    for i in range(8):
        assert lib.ral_baseline_layer_geom(variant, 2, i, row, n) == 0, lib.ral_last_error()
        got.append(tuple(row))
    assert got == rows
    for args, text in [((variant, 2, 8, row, n), b"baseline row 8 outside [0, 7]"), ((variant, 2, -1, row, n), b"baseline row -1 outside [0, 7]"),
                       ((variant, 2, 0, row, n - 1), b"baseline row: room for %d values is needed (got %d)" % (n, n - 1)),
                       ((3, 2, 0, row, n), b"baseline plan: variant must be ACDAE (4) or DANet (5), got 3")]:
        assert lib.ral_baseline_layer_geom(*args) != 0 and lib.ral_last_error() == text
    assert lib.ral_baseline_layer_geom(variant, 1, 0, row, n) != 0 and b"leads" in lib.ral_last_error()


@pytest.mark.parametrize("point", sorted(ACDAE_LAUNCHES), ids=lambda p: "%d-%d-%s" % p)
def test_acdae_launch_numbers(point):
    L, B, direction = point
    got = passplan(ACDAE, L, B, int(direction == "bwd"))
    assert [(g[1], g[2], g[3], g[5], g[6]) for g in got] == ACDAE_LAUNCHES[point]
    assert {g[4] for g in got} == {256}
    assert [g[0] for g in got] == (list(range(8)) if direction == "fwd" else [i for i in range(7, -1, -1) for _ in (0, 1)])


@pytest.mark.parametrize("point", [(L, B, d) for (L, B) in sorted(DANET_LDS) for d in ("fwd", "bwd")], ids=lambda p: "%d-%d-%s" % p)
def test_danet_launch_numbers(point):
    L, B, direction = point
    for training in ((1, 0) if direction == "fwd" else (1,)):        # a training and an eval forward launch the same
        got = passplan(DANET, L, B, int(direction == "bwd"), training)
        assert [(g[0], g[1], g[2], g[5], g[6]) for g in got] == danet_expected(L, B, direction == "bwd")
        assert {(g[3], g[4]) for g in got} == {(1, 256)}


def test_danet_grids_at_the_bench_batch():
    assert DANET_LDS[(512, 2048)]["grids"] == (1024, 128, 256, 512)


def test_sweep_of_the_legal_space():
    """every legal L of both networks at batches on both sides of every cap and of both split rules of the weight-gradient kernels"""
    lib = _lib.lib()
    chosen = set()
    for L in ACDAE_LS:
        for B in BATCHES:
            fwd, bwd = passplan(ACDAE, L, B, 0, lib=lib), passplan(ACDAE, L, B, 1, lib=lib)
            assert len(fwd) == 8 and len(bwd) == 16
            assert [e[0] for e in fwd] == list(range(8)) and [e[0] for e in bwd] == [i for i in range(7, -1, -1) for _ in (0, 1)]
            for layer, name, gx, gy, th, lds, ng in fwd + bwd:
                where = (L, B, layer, name, gx, gy, th, lds, ng)
                cin, cout, ks, convt, ish, osh, skip = ACDAE_ROWS[layer]
                lin = L >> ish
                chosen.add(name)
                assert name in ACDAE_INSTANCES and th == 256 and gx >= 1 and gy >= 1 and 0 < lds <= LDS_MAX, where
                if name.startswith("k_acd_dw"):
                    # the MFMA weight gradient iff the row has 16 or more output channels
                    assert name.startswith("k_acd_dw_m") == (cout >= 16) and name.endswith(", true>" if convt else ", false>"), where
                    blocks = -(-cout // 16) * ng if cout >= 16 else -(-cout // 8) * -(-cin // 8)
                    assert (ng == -(-(-(-cin * ks // 16)) // 16)) if cout >= 16 else ng == 0, where
                    assert gx == blocks and gy == min(max((512 if cout >= 16 else 2048) // blocks, 1), B), where
                elif name.startswith("k_acd_enc_fwd"):
                    # the MFMA encoder forward iff its tiles fit
                    mfma = cin >= 16 and cout % 32 == 0 and lin % 16 == 0
                    assert name.startswith("k_acd_enc_fwd_m") == mfma and not convt, where
                    assert (gx, gy) == ((min(B, 512), cout // 32) if mfma else (min(B, 1024), 1)) and ng == 0, where
                else:
                    assert (gx, gy, ng) == (min(B, 1024), 1, 0) and ("_dec_" in name) == bool(convt) and name.endswith("<%d>" % ks), where
            # encoder 3 leaves the MFMA form exactly when L is no multiple of 128
            assert (fwd[3][1] == "k_acd_enc_fwd<7>") == (L % 128 != 0)
    assert chosen == set(ACDAE_INSTANCES)
    chosen = set()
    for L in DANET_LS:
        for B in BATCHES:
            fwd, bwd = passplan(DANET, L, B, 0, lib=lib), passplan(DANET, L, B, 1, lib=lib)
            assert len(fwd) == 38 and len(bwd) == 38
            order = [i for i in range(8) for _ in range(6 if DANET_ROWS[i][8] else 4)]
            assert [e[0] for e in fwd] == order and [e[0] for e in bwd] == order[::-1]
            grids = {"conv": min(B, 1024), "dam1": min(B, 1024), "out": min(B, 1024), "conv_b": min(B, 1024), "fcn_mid": min(-(-B // 16), 256),
                     "fcn_bmid": min(-(-B // 16), 256), "act": min(-(-B // 4), 256), "act_b": min(-(-B // 4), 256), "dam_b": min(B, 512), "bn_b": min(B, 512)}
            prev = None
            for layer, name, gx, gy, th, lds, ng in fwd + bwd:
                where = (L, B, layer, name, gx, gy, th, lds, ng)
                cin, c, k, p, tr, ish, osh, in1, dam = DANET_ROWS[layer]
                chosen.add(name)
                assert name in DANET_INSTANCES and (gy, th) == (1, 256) and 0 <= lds <= LDS_MAX, where
                family = re.match(r"k_dn_(\w+?)(<|$)", name).group(1)
                assert gx == grids[family] and gx >= 1, where
                if family in ("fcn_mid", "fcn_bmid"):   # the DAM's fcn sits next to k_dn_dam1 / k_dn_dam_b, the APReLU's next to conv / act_b
                    assert ng == (2 if prev[:2] == (layer, "k_dn_dam1" if family == "fcn_mid" else "k_dn_dam_b") else 1), where
                    assert lds == (0 if family == "fcn_mid" else 4 * ((c * c + c) if ng == 2 else (2 * c * c + c))), where
                else:
                    assert ng == 0, where
                prev = (layer, name)
                if family in ("act", "act_b"):          # V = 4 iff the output length is a multiple of 4
                    assert name.endswith("<4>") == ((L >> osh) % 4 == 0) and lds == 0, where
                if family in ("conv", "conv_b"):
                    assert name.endswith("<%d, %s>" % (k, "true" if tr else "false")), where
                if family in ("dam1", "dam_b"):
                    assert dam, where
    assert chosen == set(DANET_INSTANCES)


def test_queries_refuse_what_a_model_refuses():
    lib = _lib.lib()
    none = (None, 0, None, None, None, None, None, None)
    for (variant, leads, L, B, k), text in [
            ((ACDAE, 1, 512, 4, 0), b"ACDAE has 2 input channels (got leads=1)"), ((ACDAE, 2, 96, 4, 0), b"ACDAE: L must be a multiple of 64 and <= 1024 (got 96)"),
            ((ACDAE, 2, 1088, 4, 0), b"ACDAE: L must be a multiple of 64 and <= 1024 (got 1088)"), ((ACDAE, 2, 0, 4, 0), b"ACDAE: L must be a multiple of 64 and <= 1024 (got 0)"),
            ((DANET, 1, 512, 4, 0), b"DANet: the last decoder cell has 2 output channels, so leads must be 2 (got 1)"),
            ((DANET, 2, 16, 4, 0), b"DANet: L must be a multiple of 16 in [32, 2048], got 16"), ((DANET, 2, 40, 4, 0), b"DANet: L must be a multiple of 16 in [32, 2048], got 40"),
            ((DANET, 2, 2064, 4, 0), b"DANet: L must be a multiple of 16 in [32, 2048], got 2064"),
            ((ACDAE, 2, 512, 0, 0), b"baseline plan: B must be positive (got 0)"), ((DANET, 2, 512, -1, 0), b"baseline plan: B must be positive (got -1)"),
            ((ACDAE, 2, 512, 4, 8), b"baseline plan: launch 8 outside [0, 8)"), ((DANET, 2, 512, 4, 38), b"baseline plan: launch 38 outside [0, 38)"),
            ((3, 2, 512, 4, 0), b"baseline plan: variant must be ACDAE (4) or DANet (5), got 3")]:
        assert lib.ral_baseline_pass_plan(variant, leads, L, B, 1, 0, k, *none) < 0
        assert lib.ral_last_error() == text
        if variant in (ACDAE, DANET) and B > 0 and k == 0:          # the same text as the model's
            cfg = _lib.make_config("acdae" if variant == ACDAE else "danet", leads, L, B, 1)
            assert lib.ral_workspace_bytes(C.byref(cfg)) < 0 and lib.ral_last_error() == text
    assert lib.ral_baseline_pass_plan(ACDAE, 2, 512, 4, 1, 1, 15, *none) == 0         # every out-pointer may be NULL
    assert lib.ral_baseline_pass_plan(ACDAE, 2, 512, 4, 1, 1, 16, *none) < 0 and lib.ral_last_error() == b"baseline plan: launch 16 outside [0, 16)"


# ---- the ledger: which instances the GPU tests that compare with the fp64 oracle or the reference's goldens launch
NOT_COVERED = {}       # instance -> why no such test runs it (none: both new ACDAE cases pass)


def parametrize_args(fn):
    return list([m for m in fn.pytestmark if m.name == "parametrize"][0].args[1])


def covering_runs():
    """[(test, variant, L, B, passes)]: a train step is a forward and a backward; DANet's tests also run an eval forward (the same
    launches as a training forward).  The golden tests run one configuration each: L = 512 at their fixture's batch."""
    import test_gpu_acdae as A
    import test_gpu_danet as D
    shapes = lambda fn: list(dict.fromkeys(c.values[0] for c in parametrize_args(fn)))      # (shape, input seed, yardstick seeds)
    runs = [("test_acdae_train_step_matches_oracle", ACDAE, L, B) for L, B in shapes(A.test_acdae_train_step_matches_oracle)]
    runs += [("test_danet_matches_fp64_oracle", DANET, L, B) for B, L, leads in shapes(D.test_danet_matches_fp64_oracle)]
    for test, variant, fixture in (("test_acdae_against_reference_golden", ACDAE, "g3_acdae_l2_L512.npz"), ("test_danet_matches_reference_golden", DANET, "g3_danet_L512.npz")):
        assert hasattr(A if variant == ACDAE else D, test)
        runs.append((test, variant, 512, np.load(os.path.join(ROOT, "tests", "golden", fixture))["x"].shape[0]))
    return runs


def launched_by(runs):
    return {e[1] for _, variant, L, B in runs for backward in (0, 1) for e in passplan(variant, L, B, backward)}


def test_the_oracle_and_golden_cases_launch_every_instance():
    """on failure: the instances no case launches - add a case for each to the oracle test of its network, or an entry with the
    reason to NOT_COVERED"""
    runs = covering_runs()
    assert {t for t, *_ in runs} == {"test_acdae_train_step_matches_oracle", "test_danet_matches_fp64_oracle", "test_acdae_against_reference_golden",
                                     "test_danet_matches_reference_golden"}
    covered = launched_by(runs)
    every = set(ACDAE_INSTANCES + DANET_INSTANCES)
    assert not set(NOT_COVERED) & covered and set(NOT_COVERED) <= every
    assert covered | set(NOT_COVERED) == every, sorted(every - covered - set(NOT_COVERED))


def test_the_ledger_is_sensitive():
    """without the two ACDAE cases whose L is no multiple of 128 exactly k_acd_enc_fwd<7> is uncovered; without DANet's L = 32 case
    the two V = 1 elementwise kernels"""
    runs = covering_runs()
    every = set(ACDAE_INSTANCES + DANET_INSTANCES)
    assert every - launched_by([r for r in runs if not (r[1] == ACDAE and r[2] % 128)]) == {"k_acd_enc_fwd<7>"}
    assert every - launched_by([r for r in runs if not (r[1] == DANET and r[2] == 32)]) == {"k_dn_act<1>", "k_dn_act_b<1>"}
