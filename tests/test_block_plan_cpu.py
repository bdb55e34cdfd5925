"""The Linear-layer dispatch of a transformer block, seen from the CPU: `ral_block_plan` (host arithmetic only) says which
kernel runs the QKV projection, the MLP half block, their backwards and the four weight-gradient products at a shape, and
these tests pin it to the first-match tables of DESIGN.md section 3, "Linear-layer dispatch": for the five levels of
L = 256, 512, 1024 and of the padded lengths L = 128, 320, in training and eval, with and without a second output, under
f16_split in {0, 32, 64, 128} x narrow_f16 in {0, 1}, under the default switches and under each option string of
tests/test_gpu_configs.py::test_narrow_level_mlp_forward_kernel_choices and of the switch runs of
tests/test_gpu_block_instances.py (a process per string: the switches latch at their first read).  The expected names below
are written out from the tables, level by level, not computed.  Names are template-ids as a kernel trace prints them, default
template arguments included: k_mlp_bwd_h<C, NCH, NTH>, k_dw<M, NC, MS, NS, LAYY, XF, H>."""
import ctypes as C
import itertools
import json
import os
import re
import subprocess
import sys

import pytest

from ecg_denoise_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parametrize_args(fn):
    """the argument list of a test function's parametrize mark"""
    return list([m for m in fn.pytestmark if m.name == "parametrize"][0].args[1])


def switch_part(opts):
    """an option string without its f16_split item: the plan query takes f16_split as an argument, so "f16_split=32,fuse_dw=0"
    reads the table of "fuse_dw=0" """
    return ",".join(kv for kv in opts.split(",") if kv and not kv.startswith("f16_split="))


def option_strings():
    """the option strings of the GPU files' child processes, read from their parametrize marks: the strip-kernel test of
    tests/test_gpu_configs.py and the switch runs of tests/test_gpu_block_instances.py"""
    import test_gpu_block_instances as inst_file   # (not at import: the child processes below import this module for its helpers)
    import test_gpu_configs as gpu_file
    both = parametrize_args(gpu_file.test_narrow_level_mlp_forward_kernel_choices) \
        + [switch_part(opts) for opts, _ in parametrize_args(inst_file.test_block_instances_under_latched_switches)]
    return list(dict.fromkeys(both))


LAUNCHES = ("qkv_fwd", "mlp_fwd", "mlp_bwd", "qkv_bwd", "dw_fc2", "dw_fc1", "dw_proj", "dw_qkv")

# ---- kernel names
QF, QWS, QH = "k_qkv_fwd<%d>", "k_qkv_fwd_ws<%d, 64>", "k_qkv_fwd_h<%d, 64>"
QB, QBH = "k_qkv_bwd<%d>", "k_qkv_bwd_h<%d>"
MF, MFH, MFW, MFWH = "k_mlp_fwd<%d, %d>", "k_mlp_fwd_h<%d, %d, %d>", "k_mlp_fwd_w<%d>", "k_mlp_fwd_wh<%d>"
MB, MBS, MBH, MBW = "k_mlp_bwd<%d, %d>", "k_mlp_bwd_s<%d, %d>", "k_mlp_bwd_h<%d, %d, %d>", "k_mlp_bwd_w<%d>"
MBW2, MBW2H = "k_mlp_bwd_w2<32, false>", "k_mlp_bwd_w2<32, true>"
# the four weight-gradient products per width (fc2, fc1, proj, qkv), without the last template argument
DW = {8: ("k_dw<8, 32, 8, 32, 0, 3, %s>", "k_dw<32, 8, 32, 8, 0, 1, %s>", "k_dw<8, 8, 8, 8, 0, 0, %s>", "k_dw<24, 8, 24, 8, 1, 2, %s>"),
      16: ("k_dw<16, 64, 16, 64, 0, 3, %s>", "k_dw<64, 16, 64, 16, 0, 1, %s>", "k_dw<16, 16, 16, 16, 0, 0, %s>", "k_dw<48, 16, 48, 16, 1, 2, %s>"),
      32: ("k_dw<32, 128, 32, 128, 0, 3, %s>", "k_dw<128, 32, 128, 32, 0, 1, %s>", "k_dw<32, 32, 32, 32, 0, 0, %s>", "k_dw<96, 32, 96, 32, 1, 2, %s>"),
      64: ("k_dw<64, 256, 64, 128, 0, 3, %s>", "k_dw<256, 64, 128, 64, 0, 1, %s>", "k_dw<64, 64, 64, 64, 0, 0, %s>", "k_dw<192, 64, 96, 64, 1, 2, %s>"),
      128: ("k_dw<128, 512, 128, 128, 0, 3, %s>", "k_dw<512, 128, 128, 128, 0, 1, %s>", "k_dw<128, 128, 128, 128, 0, 0, %s>",
            "k_dw<384, 128, 128, 128, 1, 2, %s>")}

# ---- the levels: window length -> [(C, N, NE)] (NE = 0: whole windows)
LENGTHS = {256: [(8, 256, 0), (16, 128, 0), (32, 64, 0), (64, 32, 0), (128, 16, 0)],          # (128, 16): the mixed bottom level
           512: [(8, 512, 0), (16, 256, 0), (32, 128, 0), (64, 64, 0), (128, 32, 0)],         # the bench shape
           1024: [(8, 1024, 0), (16, 512, 0), (32, 256, 0), (64, 128, 0), (128, 64, 0)],
           128: [(8, 256, 128), (16, 128, 64), (32, 64, 32), (64, 32, 16), (128, 16, 8)],     # padded: 256 slots, f16_split forced to 0
           320: [(8, 512, 320), (16, 256, 160), (32, 128, 80), (64, 64, 40), (128, 32, 20)]}   # padded: 512 slots
PADDED = (128, 320)

# ---- the tables per (C, N), default switches.  Every entry is a first-match list of (condition, kernel); the conditions
# read the point: wide = f16_split > 0 and C >= f16_split, narrow = f16_split > 0 and narrow_f16, training, second (output),
# padded.  "fused": the shape's MLP backward produces the fc1 / fc2 weight gradients (mlp_dw_fused; stores_upre is then 0);
# "split": the shapes whose data-gradient kernels publish gmax when wide (dw_split).
def _narrow_fused(Cw, nch, tw, strip_bwd):
    """a narrow level whose backward is fused: strips forward unless a second output or padded windows keep them off"""
    return {"qkv_fwd": [("", QF % Cw)],
            "mlp_fwd": [("not padded and not second and narrow", MFWH % Cw)] + ([("not padded and not second", MFW % 16)] if Cw == 16 else [])
                       + [("", MF % (Cw, nch))],
            "mlp_bwd": [("not padded", strip_bwd), ("", MBS % (Cw, tw))],
            "qkv_bwd": [("", QB % Cw)], "fused": True, "split": False}


TABLES = {
    # ---- L = 256 (and the 256 slots of L = 128)
    (8, 256): _narrow_fused(8, 1, 2, MBW % 8),
    (16, 128): _narrow_fused(16, 1, 1, MBW % 16),
    (32, 64): {"qkv_fwd": [("wide", QH % 32), ("", QF % 32)],
               "mlp_fwd": [("not padded and wide", MFH % (32, 1, 512)), ("not padded and not second and narrow", MFWH % 32), ("", MF % (32, 1))],
               "mlp_bwd": [("not padded and narrow", MBW2H), ("not padded", MBW2), ("", MBS % (32, 1))],
               "qkv_bwd": [("wide", QBH % 32), ("", QB % 32)], "fused": True, "split": False},
    (64, 32): {"qkv_fwd": [("wide", QWS % 64), ("", QF % 64)],
               "mlp_fwd": [("not padded and wide", MFH % (64, 1, 256)), ("", MF % (64, 1))],
               "mlp_bwd": [("not padded and wide", MBH % (64, 1, 512)), ("", MB % (64, 1))],          # the eight-wave form
               "qkv_bwd": [("wide", QBH % 64), ("", QB % 64)], "fused": False, "split": True},
    (128, 16): {"qkv_fwd": [("wide", QWS % 128), ("", QF % 128)],                                     # the weight-stationary projection ...
                "mlp_fwd": [("", MF % (128, 1))], "mlp_bwd": [("", MB % (128, 1))],                   # ... beside fp32 MLP kernels (N % 32 != 0)
                "qkv_bwd": [("", QB % 128)], "fused": False, "split": False},                          # ... and fp32 weight gradients
    # ---- L = 512 (and the 512 slots of L = 320)
    (8, 512): _narrow_fused(8, 2, 4, MBW % 8),
    (16, 256): _narrow_fused(16, 4, 2, MBW % 16),
    (32, 128): {"qkv_fwd": [("wide", QH % 32), ("", QF % 32)],
                "mlp_fwd": [("not padded and wide", MFH % (32, 2, 512)), ("not padded and not second and narrow", MFWH % 32), ("", MF % (32, 2))],
                "mlp_bwd": [("not padded and narrow", MBW2H), ("not padded", MBW2), ("", MBS % (32, 2))],
                "qkv_bwd": [("wide", QBH % 32), ("", QB % 32)], "fused": True, "split": False},
    (64, 64): {"qkv_fwd": [("wide", QWS % 64), ("", QF % 64)],
               "mlp_fwd": [("not padded and wide", MFH % (64, 8, 256)), ("", MF % (64, 2))],
               "mlp_bwd": [("not padded and wide", MBH % (64, 4, 256)), ("", MB % (64, 2))],          # the four-wave form: N C = 4096
               "qkv_bwd": [("wide", QBH % 64), ("", QB % 64)], "fused": False, "split": True},
    (128, 32): {"qkv_fwd": [("wide", QWS % 128), ("", QF % 128)],
                "mlp_fwd": [("not padded and wide", MFH % (128, 4, 256)), ("", MF % (128, 2))],
                "mlp_bwd": [("not padded and wide", MBH % (128, 4, 256)), ("", MB % (128, 2))],
                "qkv_bwd": [("wide", QBH % 128), ("", QB % 128)], "fused": False, "split": True},
    # ---- L = 1024: no level is fused (the tiles of k_mlp_bwd_s pass 80 KB), so training stores u_pre everywhere and the strip
    # forward runs in eval mode only; no split backward fits (N C = 8192)
    (8, 1024): {"qkv_fwd": [("", QF % 8)],
                "mlp_fwd": [("not training and not second and narrow", MFWH % 8), ("", MF % (8, 4))],
                "mlp_bwd": [("", MB % (8, 4))], "qkv_bwd": [("", QB % 8)], "fused": False, "split": False},
    (16, 512): {"qkv_fwd": [("", QF % 16)],
                "mlp_fwd": [("not training and not second and narrow", MFWH % 16), ("not training and not second", MFW % 16), ("", MF % (16, 4))],
                "mlp_bwd": [("", MB % (16, 4))], "qkv_bwd": [("", QB % 16)], "fused": False, "split": False},
    (32, 256): {"qkv_fwd": [("wide", QH % 32), ("", QF % 32)],
                "mlp_fwd": [("wide", MFH % (32, 4, 512)), ("not training and not second and narrow", MFWH % 32), ("", MF % (32, 4))],
                "mlp_bwd": [("", MB % (32, 4))], "qkv_bwd": [("", QB % 32)], "fused": False, "split": False},
    (64, 128): {"qkv_fwd": [("wide", QH % 64), ("", QF % 64)],                                        # whole windows of 128: k_qkv_fwd_h
                "mlp_fwd": [("wide", MFH % (64, 8, 256)), ("", MF % (64, 4))],
                "mlp_bwd": [("", MB % (64, 4))], "qkv_bwd": [("", QB % 64)], "fused": False, "split": False},
    (128, 64): {"qkv_fwd": [("wide", QWS % 128), ("", QF % 128)],
                "mlp_fwd": [("wide", MFH % (128, 8, 256)), ("", MF % (128, 4))],
                "mlp_bwd": [("", MB % (128, 4))], "qkv_bwd": [("", QB % 128)], "fused": False, "split": False},
}


def _with(base, **levels):
    out = dict(base)
    for key, rows in levels.items():
        Cw, N = (int(v) for v in key[1:].split("_"))
        out[(Cw, N)] = {**base[(Cw, N)], **rows}
    return out


# ---- the tables under each option string: the rows that differ from the default tables, written out level by level
EXPECTED = {
    "": TABLES,
    "tabred_side=0": TABLES,                                                                 # (schedule, not dispatch)
    # mlp_fwd_w = 0: never a strip forward; 1: fp32 strips at C = 16 only; 2: fp32 strips at every narrow width (never the f16 strips)
    # mlp_bwd_w = 0: k_mlp_bwd_s at every fused level; 1: strips at C = 16 only; 2: at C = 8 and 16; mlp_bwd_w_f16 = 0: C = 32 on fp32
    'mlp_fwd_w=0': _with(TABLES,
        _8_256={'mlp_fwd': [('', 'k_mlp_fwd<8, 1>')]},
        _16_128={'mlp_fwd': [('', 'k_mlp_fwd<16, 1>')]},
        _32_64={'mlp_fwd': [('not padded and wide', 'k_mlp_fwd_h<32, 1, 512>'), ('', 'k_mlp_fwd<32, 1>')]},
        _8_512={'mlp_fwd': [('', 'k_mlp_fwd<8, 2>')]},
        _16_256={'mlp_fwd': [('', 'k_mlp_fwd<16, 4>')]},
        _32_128={'mlp_fwd': [('not padded and wide', 'k_mlp_fwd_h<32, 2, 512>'), ('', 'k_mlp_fwd<32, 2>')]},
        _8_1024={'mlp_fwd': [('', 'k_mlp_fwd<8, 4>')]},
        _16_512={'mlp_fwd': [('', 'k_mlp_fwd<16, 4>')]},
        _32_256={'mlp_fwd': [('wide', 'k_mlp_fwd_h<32, 4, 512>'), ('', 'k_mlp_fwd<32, 4>')]}),
    'mlp_fwd_w=1': _with(TABLES,
        _8_256={'mlp_fwd': [('', 'k_mlp_fwd<8, 1>')]},
        _16_128={'mlp_fwd': [('not padded and not second', 'k_mlp_fwd_w<16>'), ('', 'k_mlp_fwd<16, 1>')]},
        _32_64={'mlp_fwd': [('not padded and wide', 'k_mlp_fwd_h<32, 1, 512>'), ('', 'k_mlp_fwd<32, 1>')]},
        _8_512={'mlp_fwd': [('', 'k_mlp_fwd<8, 2>')]},
        _16_256={'mlp_fwd': [('not padded and not second', 'k_mlp_fwd_w<16>'), ('', 'k_mlp_fwd<16, 4>')]},
        _32_128={'mlp_fwd': [('not padded and wide', 'k_mlp_fwd_h<32, 2, 512>'), ('', 'k_mlp_fwd<32, 2>')]},
        _8_1024={'mlp_fwd': [('', 'k_mlp_fwd<8, 4>')]},
        _16_512={'mlp_fwd': [('not training and not second', 'k_mlp_fwd_w<16>'), ('', 'k_mlp_fwd<16, 4>')]},
        _32_256={'mlp_fwd': [('wide', 'k_mlp_fwd_h<32, 4, 512>'), ('', 'k_mlp_fwd<32, 4>')]}),
    'mlp_fwd_w=2': _with(TABLES,
        _8_256={'mlp_fwd': [('not padded and not second', 'k_mlp_fwd_w<8>'), ('', 'k_mlp_fwd<8, 1>')]},
        _16_128={'mlp_fwd': [('not padded and not second', 'k_mlp_fwd_w<16>'), ('', 'k_mlp_fwd<16, 1>')]},
        _32_64={'mlp_fwd': [('not padded and wide', 'k_mlp_fwd_h<32, 1, 512>'), ('not padded and not second', 'k_mlp_fwd_w<32>'), ('', 'k_mlp_fwd<32, 1>')]},
        _8_512={'mlp_fwd': [('not padded and not second', 'k_mlp_fwd_w<8>'), ('', 'k_mlp_fwd<8, 2>')]},
        _16_256={'mlp_fwd': [('not padded and not second', 'k_mlp_fwd_w<16>'), ('', 'k_mlp_fwd<16, 4>')]},
        _32_128={'mlp_fwd': [('not padded and wide', 'k_mlp_fwd_h<32, 2, 512>'), ('not padded and not second', 'k_mlp_fwd_w<32>'), ('', 'k_mlp_fwd<32, 2>')]},
        _8_1024={'mlp_fwd': [('not training and not second', 'k_mlp_fwd_w<8>'), ('', 'k_mlp_fwd<8, 4>')]},
        _16_512={'mlp_fwd': [('not training and not second', 'k_mlp_fwd_w<16>'), ('', 'k_mlp_fwd<16, 4>')]},
        _32_256={'mlp_fwd': [('wide', 'k_mlp_fwd_h<32, 4, 512>'), ('not training and not second', 'k_mlp_fwd_w<32>'), ('', 'k_mlp_fwd<32, 4>')]}),
    'mlp_bwd_w=0': _with(TABLES,
        _8_256={'mlp_bwd': [('', 'k_mlp_bwd_s<8, 2>')]},
        _16_128={'mlp_bwd': [('', 'k_mlp_bwd_s<16, 1>')]},
        _32_64={'mlp_bwd': [('', 'k_mlp_bwd_s<32, 1>')]},
        _8_512={'mlp_bwd': [('', 'k_mlp_bwd_s<8, 4>')]},
        _16_256={'mlp_bwd': [('', 'k_mlp_bwd_s<16, 2>')]},
        _32_128={'mlp_bwd': [('', 'k_mlp_bwd_s<32, 2>')]}),
    'mlp_bwd_w=1': _with(TABLES,
        _8_256={'mlp_bwd': [('', 'k_mlp_bwd_s<8, 2>')]},
        _32_64={'mlp_bwd': [('', 'k_mlp_bwd_s<32, 1>')]},
        _8_512={'mlp_bwd': [('', 'k_mlp_bwd_s<8, 4>')]},
        _32_128={'mlp_bwd': [('', 'k_mlp_bwd_s<32, 2>')]}),
    'mlp_bwd_w=2': _with(TABLES,
        _32_64={'mlp_bwd': [('', 'k_mlp_bwd_s<32, 1>')]},
        _32_128={'mlp_bwd': [('', 'k_mlp_bwd_s<32, 2>')]}),
    'mlp_bwd_w_f16=0': _with(TABLES,
        _32_64={'mlp_bwd': [('not padded', 'k_mlp_bwd_w2<32, false>'), ('', 'k_mlp_bwd_s<32, 1>')]},
        _32_128={'mlp_bwd': [('not padded', 'k_mlp_bwd_w2<32, false>'), ('', 'k_mlp_bwd_s<32, 2>')]}),
    # fuse_dw = 16: C = 32 leaves the fused backward: training stores u_pre (no strip forward then), f16_split = 32 sends it to
    # k_mlp_bwd_h<32, ...> (eight waves at N = 64, four at N = 128) with split weight gradients, else to k_mlp_bwd<32, ...>
    "fuse_dw=16": _with(TABLES,
                        _32_64={"mlp_fwd": [("not padded and wide", MFH % (32, 1, 512)), ("not padded and not training and not second and narrow", MFWH % 32),
                                            ("", MF % (32, 1))],
                                "mlp_bwd": [("not padded and wide", MBH % (32, 1, 512)), ("", MB % (32, 1))], "fused": False, "split": True},
                        _32_128={"mlp_fwd": [("not padded and wide", MFH % (32, 2, 512)), ("not padded and not training and not second and narrow", MFWH % 32),
                                             ("", MF % (32, 2))],
                                 "mlp_bwd": [("not padded and wide", MBH % (32, 4, 256)), ("", MB % (32, 2))], "fused": False, "split": True}),
}
# fuse_dw = 0: no level is fused.  C = 32 as under fuse_dw = 16; C = 8 and 16 take k_mlp_bwd<C, NCH> (one hidden chunk at the
# levels of L = 256, four at those of L = 512; padded windows too), store u_pre in training and keep their strip forward for eval
# mode, with four fp32 weight-gradient products.  fuse_dw = 8: the same at C = 16 and 32, C = 8 stays fused.
EXPECTED["fuse_dw=8"] = _with(EXPECTED["fuse_dw=16"],
                              _16_128={"mlp_fwd": [("not padded and not training and not second and narrow", MFWH % 16),
                                                   ("not padded and not training and not second", MFW % 16), ("", MF % (16, 1))],
                                       "mlp_bwd": [("", MB % (16, 1))], "fused": False},
                              _16_256={"mlp_fwd": [("not padded and not training and not second and narrow", MFWH % 16),
                                                   ("not padded and not training and not second", MFW % 16), ("", MF % (16, 4))],
                                       "mlp_bwd": [("", MB % (16, 4))], "fused": False})
EXPECTED["fuse_dw=0"] = _with(EXPECTED["fuse_dw=8"],
                              _8_256={"mlp_fwd": [("not padded and not training and not second and narrow", MFWH % 8), ("", MF % (8, 1))],
                                      "mlp_bwd": [("", MB % (8, 1))], "fused": False},
                              _8_512={"mlp_fwd": [("not padded and not training and not second and narrow", MFWH % 8), ("", MF % (8, 2))],
                                      "mlp_bwd": [("", MB % (8, 4))], "fused": False})


def expected_point(tables, Cw, N, point):
    """the eight kernel names and the three flags the tables state for a point"""
    t = tables[(Cw, N)]
    first = lambda rows: next(k for cond, k in rows if not cond or eval(cond, {}, point))
    split = t["split"] and point["wide"]                      # (want_dw is 1 at every point of the tables)
    dw = [("" if t["fused"] and i < 2 else name % ("true" if split else "false")) for i, name in enumerate(DW[Cw])]
    names = [first(t["qkv_fwd"]), first(t["mlp_fwd"]), first(t["mlp_bwd"]), first(t["qkv_bwd"])] + dw
    return names, [int(point["training"] and not t["fused"]), int(t["fused"]), int(split)]


def points():
    """(L, C, N, NE, training, second_out, f16_split, narrow_f16) of the tables"""
    for Lw, levels in LENGTHS.items():
        for (Cw, N, NE), training, second, narrow in itertools.product(levels, (1, 0), (0, 1), (0, 1)):
            for f16_split in ((0,) if Lw in PADDED else (0, 32, 64, 128)):
                yield Lw, Cw, N, NE, training, second, f16_split, narrow


def plan(launch, Cw, N, NE=0, training=1, second=0, want_dw=1, f16_split=64, narrow=1, L=None):
    """(kernel name, threads, LDS bytes, chunks, split, stores_upre, mlp_dw_fused, dw_split)"""
    L = L or _lib.lib()
    name = C.create_string_buffer(96)
    th, ch, sp, su, fu, ds = (C.c_int32() for _ in range(6))
    lds = C.c_int64()
    rc = L.ral_block_plan(launch, Cw, N, NE, training, second, want_dw, f16_split, narrow, name, len(name), C.byref(th), C.byref(lds),
                          C.byref(ch), C.byref(sp), C.byref(su), C.byref(fu), C.byref(ds))
    assert rc == 0, L.ral_last_error()
    return name.value.decode(), th.value, lds.value, ch.value, sp.value, su.value, fu.value, ds.value


def model_points(Lw, f16_split):
    """(level, C, N, NE, second_out, f16_split) of the blocks of a model of window length Lw: levels are Lp >> l with Lp the next
    multiple of 256; a padded length forces f16_split 0; block 9, at level 4, is the only one with a second output"""
    Lp = -(-Lw // 256) * 256
    for l in range(5):
        for second in ((0, 1) if l == 4 else (0,)):
            yield l, 8 << l, Lp >> l, (0 if Lw == Lp else Lw >> l), second, (f16_split if Lw == Lp else 0)


def model_instances(Lw, training, f16_split, narrow, L=None):
    """the kernel instances a model of window length Lw launches under this process's switches: the eight launches of a train
    step, or the two forward launches in eval mode"""
    return {plan(i, Cw, N, NE, training, second, 1, fs, narrow, L)[0] for _, Cw, N, NE, second, fs in model_points(Lw, f16_split)
            for i in (range(8) if training else (0, 1))} - {""}


_CHILD = r"""
import ctypes as C, itertools, json, sys
sys.path.insert(0, %(tests)r)
import test_block_plan_cpu as T
from ecg_denoise_amd import _lib
_lib.apply_options(%(opts)r)
out = {"points": [], "sweep": {"n": 0, "bad": [], "refused": 0}, "reached": set()}
for Lw, Cw, N, NE, tr, so, fs, nar in T.points():
    r = [T.plan(i, Cw, N, NE, tr, so, 1, fs, nar) for i in range(8)]
    out["points"].append([[x[0] for x in r], list(r[0][5:])])
# the whole legal space: every C, N a multiple of 16 up to 1024 (a level holds C N <= 8192), the flag combinations
L = _lib.lib()
for Cw in (8, 16, 32, 64, 128):
    for N in range(16, 1025, 16):
        if Cw * N > 8192:
            out["sweep"]["refused"] += int(L.ral_block_plan(0, Cw, N, 0, 1, 0, 1, 0, 0, None, 0, *[None] * 7) != 0)
            continue
        for NE in ((0, N - 8) if N > 16 else (0,)):
            for tr, so, dw, nar in itertools.product((0, 1), repeat=4):
                for fs in ((0,) if NE else (0, 32, 64, 128)):
                    r = [T.plan(i, Cw, N, NE, tr, so, dw, fs, nar) for i in range(8)]
                    su, fu, ds = r[0][5:]
                    ok = all((x[0] == "" and i in (4, 5) and fu) or (x[1] in (128, 256, 384, 512, 768) and 0 <= x[2] <= 160 * 1024) for i, x in enumerate(r))
                    ok = ok and not (fu and su) and not (ds and not (r[2][0].startswith("k_mlp_bwd_h<") and r[3][0].startswith("k_qkv_bwd_h<")))
                    ok = ok and not (ds and not dw) and all(x[4] == ds for x in r[4:] if x[0]) and su == int(tr and not fu)
                    if not ok:
                        out["sweep"]["bad"].append([Cw, N, NE, tr, so, dw, fs, nar, r])
                    out["sweep"]["n"] += 1
                    out["reached"].update(x[0] for x in r)
out["reached"] = sorted(out["reached"])
out["sweep"]["bad"] = out["sweep"]["bad"][:5]
print(json.dumps(out))
"""


def _child(opts):
    code = _CHILD % {"tests": os.path.join(ROOT, "tests"), "opts": opts}
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def seen():
    """option string -> what a fresh process with these switches sees (the default switches included)"""
    return {opts: _child(opts) for opts in EXPECTED}


def test_the_expected_tables_cover_the_gpu_file():
    assert set(EXPECTED) == {""} | set(option_strings())
    for tables in EXPECTED.values():
        assert set(tables) == {(Cw, N) for levels in LENGTHS.values() for Cw, N, _ in levels}


@pytest.mark.parametrize("opts", list(EXPECTED))
def test_kernel_names_and_flags_of_the_model_levels(seen, opts):
    got = seen[opts]["points"]
    wrong = []
    for (Lw, Cw, N, NE, tr, so, fs, nar), (names, flags) in zip(points(), got):
        point = {"wide": fs > 0 and Cw >= fs, "narrow": fs > 0 and bool(nar), "training": bool(tr), "second": bool(so), "padded": NE > 0}
        want = expected_point(EXPECTED[opts], Cw, N, point)
        if [names, flags] != list(want):
            wrong.append(((Lw, Cw, N, NE, tr, so, fs, nar), dict(zip(LAUNCHES, zip(names, want[0]))), flags, want[1]))
    assert len(got) == len(list(points())) and not wrong, (opts, len(wrong), wrong[:3])


def test_every_kernel_instance_is_reached(seen):
    """Coverage closure: every enumerator of BlockKernel (csrc/ral_block_plan.hpp) is chosen at some point of the legal space
    under some option string - an instance nothing reaches is dead code.  (Chosen somewhere in the space is not yet launched by
    a model, nor compared with the oracle: tests/test_block_coverage_cpu.py, the ledger, counts which instances a model can
    launch and which GPU test compares each with the fp64 oracle; tests/test_gpu_block_instances.py holds the cases for the
    instances the other parity tests do not reach.)"""
    hpp = open(os.path.join(ROOT, "ecg_denoise_amd", "csrc", "ral_block_plan.hpp")).read()
    every = dict(re.findall(r'^\s*X\((\w+), "([^"]+)"\)', hpp, flags=re.M))
    assert len(every) >= 100 and len(set(every.values())) == len(every)
    reached = {name for s in seen.values() for name in s["reached"]} - {""}
    assert set(every.values()) - reached == set(), sorted(set(every.values()) - reached)
    assert reached <= set(every.values())


@pytest.mark.parametrize("opts", list(EXPECTED))
def test_plan_sweep_is_launchable_and_consistent(seen, opts):
    """every point of the legal space: threads in {128, 256, 384, 512, 768}, at most 160 KB of LDS, mlp_dw_fused implies not
    stores_upre, dw_split implies the _h data-gradient kernels (and want_dw, and split products).  The query refuses exactly
    the (C, N) no level of a model can have: C N > 8192 floats per window (a level holds 8 Lp, Lp <= 1024)."""
    s = seen[opts]["sweep"]
    assert s["bad"] == [] and s["n"] > 9000
    assert s["refused"] == sum(1 for Cw in (8, 16, 32, 64, 128) for N in range(16, 1025, 16) if Cw * N > 8192)


def test_workspace_size_agrees_with_stores_upre():
    """ral_workspace_bytes of a training handle holds 4 E floats of u_pre (E = 8 Lp B floats) for every block whose plan says
    stores_upre, summed over the 18 blocks (two per stage; stage levels 0 1 2 3 4 4 3 2 1), and nothing else that is not linear
    in the slots per window Lp."""
    L = _lib.lib()
    stage_levels = (0, 1, 2, 3, 4, 4, 3, 2, 1)
    def storing_blocks(Lp):
        return sum(2 * plan(1, 8 << l, Lp >> l, 0, 1, 0, 1, 0, 0)[5] for l in stage_levels)
    assert [storing_blocks(Lp) for Lp in (256, 512, 768, 1024)] == [8, 8, 18, 18]   # (the four stages of levels 3 and 4 store; at 768 and 1024 every stage)
    B = 4
    for variant in (0, 1, 2):
        size = {Lw: L.ral_workspace_bytes(C.byref(_lib.RalConfig(variant, 2, Lw, B, 1))) for Lw in (256, 512, 768, 1024)}
        assert all(v > 0 for v in size.values())
        # per block: 4 E floats of u_pre; everything else of the workspace is linear in Lp between 256-multiples with the same
        # constants (tensors of E, 3 E, E / 4, E / 8 floats - whole multiples of 256 bytes at B = 4), so the second difference of
        # the size over Lp = 256, 512, 768, 1024 isolates the storing blocks
        upre = lambda Lp: storing_blocks(Lp) * 4 * 8 * Lp * B * 4
        rest = {Lp: size[Lp] - upre(Lp) for Lp in size}
        assert rest[512] - rest[256] == rest[768] - rest[512] == rest[1024] - rest[768], (variant, size, rest)


def test_plan_query_validates_like_the_attention_query():
    L = _lib.lib()
    tail = (None, 0) + (None,) * 7
    bad = [(0, 24, 64, 0, 1, 0, 1, 64, 1), (0, 64, 24, 0, 1, 0, 1, 64, 1), (0, 64, 1040, 0, 1, 0, 1, 64, 1), (0, 64, 64, 65, 1, 0, 1, 0, 1),
           (0, 64, 64, -1, 1, 0, 1, 0, 1), (8, 64, 64, 0, 1, 0, 1, 64, 1), (-1, 64, 64, 0, 1, 0, 1, 64, 1), (0, 128, 128, 0, 1, 0, 1, 64, 1),
           (0, 64, 64, 40, 1, 0, 1, 64, 1), (0, 64, 64, 0, 1, 0, 1, -1, 1)]
    for args in bad:
        assert L.ral_block_plan(*args, *tail) != 0 and L.ral_last_error(), args
    assert L.ral_block_plan(2, 64, 64, 0, 1, 0, 1, 64, 1, *tail) == 0            # every out-pointer is optional
    name = C.create_string_buffer(8)
    assert L.ral_block_plan(2, 64, 64, 0, 1, 0, 1, 64, 1, name, len(name), *(None,) * 7) == 0
    assert name.value == b"k_mlp_b"                                               # truncated, terminated
    assert plan(2, 64, 64)[0] == MBH % (64, 4, 256) and plan(4, 16, 256)[0] == ""   # (a product the MLP backward produced)
    assert plan(2, 64, 64, want_dw=0)[7] == 0 and plan(2, 64, 64)[7] == 1          # no weight gradients: nothing publishes gmax
