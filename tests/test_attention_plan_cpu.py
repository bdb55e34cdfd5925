"""The attention dispatch, seen from the CPU: `ral_attention_plan` (host arithmetic only) says which kernel
ral_attention_forward / _backward run for a shape, and these tests pin it to the two tables of DESIGN.md section 3 for every
case of tests/test_gpu_attention.py - under the default switches and under each option string of its
`test_every_kernel_choice_of_the_launchers` (a process per string: the switches latch at their first read).  The expected
names below are written out from the tables, not computed.  Names are template-ids as a kernel trace prints them, default
template arguments included: k_attn_fwd<QT, NT, TAB, F16, RAG>, k_attn_bwd<QT, NT, TAB, RAG>."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

import test_gpu_attention as gpu_file
from ecg_denoise_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(test, index=0):
    marks = [m for m in test.pytestmark if m.name == "parametrize"]
    return list(marks[index].args[1])


# every (N, H, Len) the GPU file runs (the kernel does not depend on the batch), in the order of its lists
CASES = list(dict.fromkeys(
    [(N, H, Len) for N, H, Len, _ in _params(gpu_file.test_attention_operator_against_fp64)]
    + [c for m in gpu_file.test_attention_operator_operand_ranges.pytestmark if m.args[0] == "N,H,Len" for c in m.args[1]]
    + _params(gpu_file.test_attention_operator_many_windows)))
OPTION_STRINGS = _params(gpu_file.test_every_kernel_choice_of_the_launchers)

# forward
T32, T32T = "k_attn_fwd_t32<2, false>", "k_attn_fwd_t32<2, true>"
FV, FVT = "k_attn_fwd_v<false>", "k_attn_fwd_v<true>"
FG1, FG2 = "k_attn_fwd<1, 0, true, false, false>", "k_attn_fwd<2, 0, true, false, false>"
FG2H, FG2N32 = "k_attn_fwd<2, 0, true, true, false>", "k_attn_fwd<2, 32, false, false, false>"
fw = lambda n, tab, f16: "k_attn_fwd_w<%d, %s, %s>" % (n, str(tab).lower(), str(f16).lower())
# backward
bm = lambda n, tab: "k_attn_bwd_m<%d, %s>" % (n, str(tab).lower())
bw = lambda n, tab: "k_attn_bwd_w<%d, %s>" % (n, str(tab).lower())
MH4, MH4T, MH8, MH8T = ("k_attn_bwd_mh<%s>" % a for a in ("4, false", "4, true", "8, false", "8, true"))
BG1, BG2 = "k_attn_bwd<1, 0, true, false>", "k_attn_bwd<2, 0, true, false>"
BG2N32, BG2N64T = "k_attn_bwd<2, 32, false, false>", "k_attn_bwd<2, 64, true, false>"
BV = "k_attn_bwd_vq + k_attn_bwd_vkv"

# ---- forward table, per switch setting that changes it: (N, H, Len) -> kernel
FWD_DEFAULT = {   # f16, attn_fwd_w = 1, attn_fwd_h = attn_fwd_t32 = 256
    (512, 2, 32): T32T, (256, 4, 16): T32T, (1024, 2, 64): T32T, (256, 4, 0): T32, (512, 2, 0): T32, (1024, 1, 0): T32,     # row 3
    (128, 8, 8): FVT, (64, 16, 4): FVT, (64, 2, 32): FVT, (128, 8, 0): FV, (64, 16, 0): FV,                                   # row 4
    (32, 32, 0): fw(32, False, True), (32, 8, 8): fw(32, True, True), (32, 2, 24): fw(32, True, True),                        # row 2
    (288, 2, 0): FG2H,     # row 5: f16 tile, N % 64 != 0 keeps it from row 3
    (48, 8, 8): FG1,       # row 6
}
FWD_STRICT = {**FWD_DEFAULT, **{   # attn_f16 = 0: no row 3, no f16 tile
    (512, 2, 32): FG2, (512, 2, 0): FG2, (288, 2, 0): FG2,       # row 5 (HG = 2)
    (1024, 2, 64): FG2, (1024, 1, 0): FG2,                       # row 6 (one head fills the LDS budget: HG = 1)
    (256, 4, 16): FVT, (256, 4, 0): FV,                          # row 4 takes N = 256 again
    (32, 32, 0): fw(32, False, False), (32, 8, 8): fw(32, True, False), (32, 2, 24): fw(32, True, False),
}}
FWD_NO_W_NO_H = {**FWD_DEFAULT, **{   # attn_fwd_w = 0, attn_fwd_h = 0 (f16, row 3 still on)
    (32, 32, 0): FG2N32, (32, 8, 8): FG2, (32, 2, 24): FG2, (288, 2, 0): FG2,
}}
_W2 = [(128, 8, 8), (64, 16, 4), (64, 2, 32), (128, 8, 0), (64, 16, 0)]   # attn_fwd_w = 2: row 2 takes N = 64 and 128 too
FWD_W2 = {**FWD_DEFAULT, **{c: fw(c[0], c[2] > 0, True) for c in _W2}}
FWD_W2_STRICT = {**FWD_STRICT, **{c: fw(c[0], c[2] > 0, False) for c in _W2}}

# ---- backward table
BWD_DEFAULT = {   # f16, every family on
    (128, 8, 8): bm(128, True), (64, 16, 4): bm(64, True), (64, 2, 32): bm(64, True), (32, 8, 8): bm(32, True),
    (32, 2, 24): bm(32, True), (32, 32, 0): bm(32, False), (128, 8, 0): bm(128, False), (64, 16, 0): bm(64, False),           # row 2
    (512, 2, 32): MH4T, (256, 4, 16): MH4T, (256, 4, 0): MH4, (512, 2, 0): MH4, (1024, 2, 64): MH8T, (1024, 1, 0): MH8,      # row 3
    (288, 2, 0): BG2,      # row 6 (N is no whole number of the one-sweep kernel's key tiles)
    (48, 8, 8): BG1,       # row 7
}
_LONG = [(512, 2, 32), (256, 4, 16), (256, 4, 0), (512, 2, 0), (1024, 2, 64), (1024, 1, 0)]
BWD_NO_M = {**BWD_DEFAULT, **{c: BG2 for c in _LONG}}   # strict mode, or attn_bwd_m = attn_bwd_mh = 0: rows 4, 6, 7
BWD_NO_M.update({c: bw(c[0], c[2] > 0) for c in BWD_DEFAULT if c[0] in (32, 64, 128)})
BWD_TILES = {**BWD_NO_M, **{   # attn_bwd_w = 0 as well: rows 5, 6
    (128, 8, 0): BV, (64, 16, 0): BV,
    (64, 16, 4): BG2N64T, (64, 2, 32): BG2N64T, (32, 32, 0): BG2N32, (128, 8, 8): BG2, (32, 8, 8): BG2, (32, 2, 24): BG2,
}}

EXPECTED = {
    "": (FWD_DEFAULT, BWD_DEFAULT),
    "attn_f16=0": (FWD_STRICT, BWD_NO_M),
    "attn_bwd_m=0,attn_bwd_mh=0": (FWD_DEFAULT, BWD_NO_M),
    "attn_bwd_m=0,attn_bwd_mh=0,attn_bwd_w=0,attn_fwd_w=0,attn_fwd_h=0": (FWD_NO_W_NO_H, BWD_TILES),
    "attn_fwd_w=2": (FWD_W2, BWD_DEFAULT),
    "attn_fwd_w=2,attn_f16=0": (FWD_W2_STRICT, BWD_NO_M),
}


def plan(backward, N, H, Len, f16=-1, NE=0, B=3):
    """(kernel name, heads per item, threads, LDS bytes, scratch floats)"""
    name = C.create_string_buffer(96)
    hg, threads, lds, scratch = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
    rc = _lib.lib().ral_attention_plan(backward, N, H, Len, int(Len > 0), f16, NE, B, name, len(name), C.byref(hg), C.byref(threads),
                                       C.byref(lds), C.byref(scratch))
    assert rc == 0, _lib.lib().ral_last_error()
    return name.value.decode(), hg.value, threads.value, lds.value, scratch.value


def _names_in_child(opts):
    """{"N,H,Len": [forward, backward]} as a fresh process with these switches sees it"""
    code = ("import ctypes as C, json\n"
            "from ecg_denoise_amd import _lib\n"
            "_lib.apply_options(%r)\n"
            "def name(backward, N, H, Len):\n"
            "    buf = C.create_string_buffer(96)\n"
            "    assert _lib.lib().ral_attention_plan(backward, N, H, Len, int(Len > 0), -1, 0, 3, buf, 96, None, None, None, None) == 0\n"
            "    return buf.value.decode()\n"
            "print(json.dumps({'%%d,%%d,%%d' %% c: [name(0, *c), name(1, *c)] for c in %r}))\n" % (opts, CASES))
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return {tuple(int(x) for x in k.split(",")): tuple(v) for k, v in json.loads(p.stdout.strip().splitlines()[-1]).items()}


def test_the_expected_tables_cover_the_gpu_file():
    assert set(EXPECTED) == {""} | set(OPTION_STRINGS)
    for fwd, bwd in EXPECTED.values():
        assert set(fwd) == set(CASES) and set(bwd) == set(CASES)


@pytest.fixture(scope="module")
def chosen():
    """option string -> {(N, H, Len): (forward, backward)}; a process each, the default switches included"""
    return {opts: _names_in_child(opts) for opts in EXPECTED}


@pytest.mark.parametrize("opts", list(EXPECTED))
def test_kernel_names_of_the_gpu_cases(chosen, opts):
    fwd, bwd = EXPECTED[opts]
    got = chosen[opts]
    wrong = {c: (got[c], (fwd[c], bwd[c])) for c in CASES if got[c] != (fwd[c], bwd[c])}
    assert not wrong, (opts, wrong)


def test_every_kernel_is_reached_by_the_gpu_file(chosen):
    """Coverage closure: every enumerator of AttnKernel (csrc/ral_attn_plan.hpp) is what some (case, option string) of
    tests/test_gpu_attention.py runs - a family nothing reaches is dead code or lacks a case there.  The two padded-window
    kernels are reached through a model whose L is no multiple of 256:
    tests/test_gpu_parity.py::test_window_lengths_that_are_multiples_of_16_match_oracle."""
    hpp = open(os.path.join(ROOT, "ecg_denoise_amd", "csrc", "ral_attn_plan.hpp")).read()
    every = dict(re.findall(r'^\s*X\((\w+), "([^"]+)"\)', hpp, flags=re.M))
    assert len(every) >= 40 and len(set(every.values())) == len(every)
    padded = {every.pop("FWD_RAG"), every.pop("BWD_RAG")}
    assert padded == {plan(0, 192, 8, 8, NE=144)[0], plan(1, 192, 8, 8, NE=144)[0]}
    reached = {name for got in chosen.values() for pair in got.values() for name in pair}
    assert set(every.values()) - reached == set(), sorted(set(every.values()) - reached)
    assert reached <= set(every.values())


def test_plan_sweep_is_launchable_and_sized_like_the_scratch_query():
    """every legal shape has a plan a gfx950 workgroup can hold, the scratch it states is what the size query tells callers,
    and it grows at most linearly with the batch (what lets ral_create check one window's share of the workspace)"""
    L = _lib.lib()
    n = 0
    for N in range(16, 1025, 16):
        for H in (1, 2, 4, 8, 16, 32):
            for Len in (0, 32, 16, 8, 4):          # none, or a centred table of the model's lengths
                if Len > N:
                    continue
                for f16 in (0, 1):
                    for backward in (0, 1):
                        per_window = plan(backward, N, H, Len, f16, B=1)[4]
                        for B in (1, 3, 700, 2048):
                            name, hg, threads, lds, scratch = plan(backward, N, H, Len, f16, B=B)
                            assert name and 1 <= hg <= H and threads in (256, 512) and 0 <= lds <= 160 * 1024, (N, H, Len, f16, B, name)
                            assert scratch <= B * per_window and (backward or scratch == 0), (N, H, Len, f16, B, name)
                            n += 1
                for B in (1, 3, 700, 2048):
                    assert plan(1, N, H, Len, -1, B=B)[4] == L.ral_attention_backward_scratch_floats(N, H, Len, int(Len > 0), B)
    assert n == (64 * 5 - 1) * 6 * 2 * 2 * 4   # (N = 16 has no 32-token table)


def test_plan_query_validates_like_the_operator():
    L = _lib.lib()
    bad = [(0, 24, 2, 0, 0, -1, 0, 1), (0, 64, 3, 0, 0, -1, 0, 1), (1, 64, 2, 9, 1, -1, 0, 1), (1, 64, 2, 0, 0, -1, 0, 0),
           (0, 64, 2, 0, 0, -1, 65, 1)]
    for args in bad:
        assert L.ral_attention_plan(*args, None, 0, None, None, None, None) != 0 and L.ral_last_error(), args
    assert L.ral_attention_plan(1, 64, 16, 4, 1, -1, 0, 4, None, 0, None, None, None, None) == 0   # every out-pointer is optional
    name = C.create_string_buffer(8)
    assert L.ral_attention_plan(1, 64, 16, 4, 1, 1, 0, 4, name, len(name), None, None, None, None) == 0
    assert name.value == b"k_attn_"                                                                 # truncated, terminated
