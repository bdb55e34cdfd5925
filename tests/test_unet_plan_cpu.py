"""U-Net stage dispatch (csrc/ral_unet_plan.*) on the CPU, through `ral_unet_stage_plan` / `ral_unet_stage_geom` alone: the stage
table and the kernel names against tables written out here, launch numbers worked out by hand from the formulas the launchers
had before the plan existed, a sweep of the legal space for what every launch must satisfy, and the ledger: the cases of
tests/test_gpu_unet.py::test_unet_train_step_matches_oracle (a train step, then an eval forward, both against the fp64 oracle)
launch every one of the 28 kernel instances."""
import ctypes as C
import os
import re

import pytest

from ecg_denoise_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("eval", "train", "bwd")          # stage-by-stage eval forward, training forward, backward
BATCHES = (1, 2, 3, 37, 511, 512, 513, 1025, 2048, 4096)
GRID_CAP = 512                            # every direction (the eval cap is the switch UNET_EVAL_GRID, default 512)

FT, BT = "k_unet_fwd_t<%s>", "k_unet_bwd_t<%s>"
# <CIN, COUT, KS, MODE> per stage, leads = 2 / 1 (stages 0 and 10 differ)
T_ARGS = {2: ("2, 4, 3, 0", "4, 8, 3, 0", "8, 16, 3, 0", "16, 32, 3, 0", "32, 32, 1, 1", "32, 32, 3, 1", "32, 32, 1, 1", "32, 16, 4, 2",
              "16, 8, 4, 2", "8, 4, 4, 2", "4, 2, 4, 2"),
          1: ("1, 4, 3, 0", "4, 8, 3, 0", "8, 16, 3, 0", "16, 32, 3, 0", "32, 32, 1, 1", "32, 32, 3, 1", "32, 32, 1, 1", "32, 16, 4, 2",
              "16, 8, 4, 2", "8, 4, 4, 2", "4, 1, 4, 2")}
INSTANCES = (["k_unet_fwd", "k_unet_bwd", "k_unet_infer<1>", "k_unet_infer<2>"]
             + [f % a for f in (FT, BT) for a in ("1, 4, 3, 0", "2, 4, 3, 0", "4, 8, 3, 0", "8, 16, 3, 0", "16, 32, 3, 0", "32, 32, 1, 1", "32, 32, 3, 1",
                                                  "32, 16, 4, 2", "16, 8, 4, 2", "8, 4, 4, 2", "4, 1, 4, 2", "4, 2, 4, 2")])


# ---- the stage table: cin cout ks mode stride pad type post_lrelu bn | a: z act accumulate | b | r | len_shift
# (z: -1 absent, -2 the input x; mode 0 conv, 1 bottleneck conv, 2 transposed; type 0 z -> BN -> [lrelu], 1 lrelu(z) -> BN, 2 no BN)
def stage_rows(leads):
    no = (-1, 0, 0)
    return [
        (leads, 4, 3, 0, 2, 1, 0, 0, 0) + (-2, 0, 0) + no + no + (1,),
        (4, 8, 3, 0, 2, 1, 0, 0, 1) + (0, 1, 1) + no + no + (2,),
        (8, 16, 3, 0, 2, 1, 0, 0, 2) + (1, 1, 1) + no + no + (3,),
        (16, 32, 3, 0, 2, 1, 0, 0, 3) + (2, 1, 1) + no + no + (4,),
        (32, 32, 1, 1, 1, 0, 1, 1, 4) + (3, 1, 1) + no + no + (4,),
        (32, 32, 3, 1, 1, 1, 1, 1, 5) + (4, 0, 0) + no + no + (4,),
        (32, 32, 1, 1, 1, 0, 2, 0, -1) + (5, 0, 0) + no + (3, 1, 0) + (4,),
        (32, 16, 4, 2, 1, 0, 0, 0, 6) + (6, 0, 0) + no + no + (3,),
        (16, 8, 4, 2, 1, 0, 0, 0, 7) + (7, 1, 0) + (2, 1, 0) + no + (2,),
        (8, 4, 4, 2, 1, 0, 0, 0, 8) + (8, 1, 0) + (1, 1, 0) + no + (1,),
        (4, leads, 4, 2, 1, 0, 0, 0, 9) + (9, 1, 0) + (0, 1, 0) + no + (0,),
    ]


# ---- (grid, windows per pass, threads, LDS bytes) per stage, by hand from the launchers' formulas before the plan:
#   forward  WP = ceil(B / min(B, 512)) capped at 4, one less while LDS > 80 KB; grid = min(ceil(B / WP), min(B, 512));
#            floats = WP cin (lin + 8) + [stage 6: WP cout lout] + cout (cin ks + 4) + 552
#   backward WP capped at 2, then 1 while LDS > 80 KB; grid = min(B, 512);
#            floats = WP cin (lin + 8) (1 + [si > 0] + [skip operand or accumulating]) + WP cout (lout + 10) + 2 cin cout ks + 4 cin + 1004
#   generic  grid = min(B, 512), 256 threads; forward floats = cin lin + cin cout ks + 488, backward 2 cin lin + cout lout + cin cout ks + 936
# e.g. (2, 512, 2048) forward stage 0: WP 4: 4 * 2 * 520 + 4 * 10 + 552 = 4752 floats = 19008 bytes
FWD_2_512_2048 = [(512, 4, 512, 19008), (512, 4, 512, 19616), (512, 4, 512, 21408), (512, 4, 512, 27296), (512, 4, 512, 27296), (512, 4, 512, 35488),
                  (512, 4, 512, 43680), (512, 4, 512, 31136), (512, 4, 512, 22816), (512, 4, 512, 20192), (512, 4, 512, 19264)]
# (2, 2048, 1100): three windows per pass are asked for (1100 / 512); forward stage 6 (32 channels in, out and residual tiles) is cut to
# two (3: 107 424 bytes), so its grid is min(550, 512); backward: every stage but 0 is cut from two to one
FWD_2_2048_1100 = [(367, 3, 512, 51712), (367, 3, 512, 52256), (367, 3, 512, 53920), (367, 3, 512, 59552), (367, 3, 512, 59040), (367, 3, 512, 67232),
                   (512, 2, 512, 74400), (367, 3, 512, 62880), (367, 3, 512, 55072), (367, 3, 512, 52704), (367, 3, 512, 51904)]
# (2, 64, 1025): 342 workgroups of three windows, the last pass of the last one holds two
FWD_2_64_1025 = [(342, 3, 512, 4096), (342, 3, 512, 4640), (342, 3, 512, 6304), (342, 3, 512, 11936), (342, 3, 512, 11424), (342, 3, 512, 19616),
                 (342, 3, 512, 12960), (342, 3, 512, 15264), (342, 3, 512, 7456), (342, 3, 512, 5088), (342, 3, 512, 4288)]
FWD_LDS_2_512_WP1 = (6528, 6944, 8352, 13472, 11936, 20128, 16032, 15776, 8992, 7136, 6592)
BWD_LDS_2_512_WP1 = (12656, 21936, 25008, 35760, 33456, 44720, 28336, 35888, 26608, 22480, 21184)
LAUNCHES = {
    (2, 512, 2048, "train"): FWD_2_512_2048,
    (2, 512, 2048, "eval"): FWD_2_512_2048,
    (2, 512, 2048, "bwd"): [(512, 2, 512, 21072), (512, 2, 512, 39024), (512, 2, 512, 42800), (512, 2, 512, 54960), (512, 2, 512, 54192), (512, 2, 512, 60336),
                            (512, 2, 512, 43952), (512, 2, 512, 50864), (512, 2, 512, 44848), (512, 2, 512, 39792), (512, 2, 512, 38032)],
    (2, 2048, 1100, "train"): FWD_2_2048_1100,
    (2, 2048, 1100, "eval"): FWD_2_2048_1100,
    (2, 2048, 1100, "bwd"): [(512, 2, 512, 70224), (512, 1, 512, 71088), (512, 1, 512, 74160), (512, 1, 512, 84912), (512, 1, 512, 82608), (512, 1, 512, 81584),
                             (512, 1, 512, 65200), (512, 1, 512, 72752), (512, 1, 512, 75760), (512, 1, 512, 71632), (512, 1, 512, 70336)],
    (2, 64, 1025, "train"): FWD_2_64_1025,
    (2, 64, 1025, "eval"): FWD_2_64_1025,
    (2, 64, 1025, "bwd"): [(512, 2, 512, 6736), (512, 2, 512, 10352), (512, 2, 512, 14128), (512, 2, 512, 26288), (512, 2, 512, 25520), (512, 2, 512, 38832),
                           (512, 2, 512, 22448), (512, 2, 512, 29360), (512, 2, 512, 16176), (512, 2, 512, 11120), (512, 2, 512, 9360)],
    (2, 512, 1, "train"): [(1, 1, 512, b) for b in FWD_LDS_2_512_WP1],
    (2, 512, 1, "eval"): [(1, 1, 512, b) for b in FWD_LDS_2_512_WP1],
    (2, 512, 1, "bwd"): [(1, 1, 512, b) for b in BWD_LDS_2_512_WP1],
    (2, 512, 3, "train"): [(3, 1, 512, b) for b in FWD_LDS_2_512_WP1],
    (2, 512, 3, "eval"): [(3, 1, 512, b) for b in FWD_LDS_2_512_WP1],
    (2, 512, 3, "bwd"): [(3, 1, 512, b) for b in BWD_LDS_2_512_WP1],
    # L = 48: stages 2 - 8 run the generic kernels (256 threads, one window per pass)
    (2, 48, 5, "train"): [(5, 1, 512, 2816), (5, 1, 512, 3232), (5, 1, 256, 3872), (5, 1, 256, 8480), (5, 1, 256, 6432), (5, 1, 256, 14624), (5, 1, 256, 6432),
                          (5, 1, 256, 10528), (5, 1, 256, 4384), (5, 1, 512, 3424), (5, 1, 512, 2880)],
    (2, 48, 5, "bwd"): [(5, 1, 512, 5232), (5, 1, 512, 7088), (5, 1, 256, 6432), (5, 1, 256, 11040), (5, 1, 256, 8992), (5, 1, 256, 17184), (5, 1, 256, 8992),
                        (5, 1, 256, 13088), (5, 1, 256, 6944), (5, 1, 512, 7632), (5, 1, 512, 6336)],
}


def query(mode, leads, L, B, si, fused=1, lib=None):
    """(kernel name, grid, windows per pass, threads, LDS bytes, fold, fused_eval)"""
    lib = lib or _lib.lib()
    name = C.create_string_buffer(64)
    grid, th, wp, fold, fe = (C.c_int32() for _ in range(5))
    lds = C.c_int64()
    rc = lib.ral_unet_stage_plan(int(mode == "bwd"), leads, L, B, int(mode != "eval"), si, fused, name, len(name), C.byref(grid), C.byref(th),
                                 C.byref(wp), C.byref(lds), C.byref(fold), C.byref(fe))
    assert rc == 0, lib.ral_last_error()
    return name.value.decode(), grid.value, wp.value, th.value, lds.value, fold.value, fe.value


def expected_names(leads, L, mode):
    """levels L / 2 .. L / 16; a stage is specialised iff its input and output lengths are multiples of 4"""
    fmt, generic = (BT, "k_unet_bwd") if mode == "bwd" else (FT, "k_unet_fwd")
    if L == 48:      # levels 24 / 12 / 6 / 3
        special = (0, 1, 9, 10)
    else:
        assert L in (512, 320, 256, 1024, 64, 2048)
        special = range(11)
    return [fmt % T_ARGS[leads][si] if si in special else generic for si in range(11)]


def test_the_instance_list_is_the_28_of_the_header():
    hpp = open(os.path.join(ROOT, "ecg_denoise_amd", "csrc", "ral_unet_plan.hpp")).read()
    listed = re.findall(r'^\s*X\(\w+, "([^"]+)"\)', hpp, flags=re.M)
    assert len(INSTANCES) == 28 and sorted(listed) == sorted(INSTANCES)


@pytest.mark.parametrize("leads", [1, 2])
def test_stage_table(leads):
    lib = _lib.lib()
    row = (C.c_int32 * 19)()
    got = []
    for si in range(11):
        assert lib.ral_unet_stage_geom(leads, si, row, 19) == 0, lib.ral_last_error()
        got.append(tuple(row))
        assert lib.ral_unet_stage_bn(si) == got[-1][8]
    assert got == stage_rows(leads)
    assert lib.ral_unet_stage_geom(leads, 11, row, 19) != 0 and lib.ral_unet_stage_geom(3, 0, row, 19) != 0 and lib.ral_unet_stage_geom(leads, 0, row, 18) != 0


@pytest.mark.parametrize("leads,L,fold", [(2, 512, 1), (1, 512, 1), (2, 48, 0), (1, 48, 0), (2, 320, 1)])
def test_kernel_names(leads, L, fold):
    for mode in MODES:
        got = [query(mode, leads, L, 5, si) for si in range(11)]
        assert [g[0] for g in got] == expected_names(leads, L, mode), (mode, got)
        assert {g[5] for g in got} == {fold}
        assert {g[6] for g in got} == {1 if L == 512 else 0}


def test_fused_eval_lengths_and_the_pass_level_answer():
    for leads in (1, 2):
        for L in range(16, 2049, 16):
            on, off = query("eval", leads, L, 7, -1, fused=1), query("eval", leads, L, 7, -1, fused=0)
            assert on[6] == (1 if L in (256, 512, 768, 1024) else 0) and off[6] == 0, L
            assert on[5] == off[5] == (1 if L % 64 == 0 else 0)
            # the fused kernel: 256 threads, grid 0 = "the workgroups resident at once" (a device question); else no kernel
            assert on[:4] == (("k_unet_infer<%d>" % leads, 0, 1, 256) if on[6] else ("", 0, 0, 0)), (L, on)
            assert off[:5] == ("", 0, 0, 0, 0)
            # a training forward or a backward pass is never one kernel
            assert query("train", leads, L, 7, -1)[:5] == ("", 0, 0, 0, 0) and query("bwd", leads, L, 7, -1)[:5] == ("", 0, 0, 0, 0)
    # LDS floats of a window's tensors, by hand at L = 512: 4 (256 + 8) + 32 * 100 + 128 * 8 + 64 * 16 + 33 * 68 + 32 * 72 + 65 * 36 + 288 + 512
    assert query("eval", 2, 512, 2048, -1)[4] == 4 * (1056 + 3200 + 1024 + 1024 + 2244 + 2304 + 2340 + 288 + 512)


@pytest.mark.parametrize("point", sorted(LAUNCHES), ids=lambda p: "%d-%d-%d-%s" % p)
def test_launch_numbers(point):
    leads, L, B, mode = point
    got = [query(mode, leads, L, B, si) for si in range(11)]
    assert [g[1:5] for g in got] == LAUNCHES[point]
    assert [g[0] for g in got] == expected_names(leads, L, mode)


def test_sweep_every_launch_is_launchable_and_consistent():
    lib = _lib.lib()
    for leads in (1, 2):
        rows = stage_rows(leads)
        for L in range(16, 2049, 16):
            for B in BATCHES:
                bwd_grids = set()
                for mode in MODES:
                    for si in range(11):
                        name, grid, wp, th, lds, fold, fe = query(mode, leads, L, B, si, lib=lib)
                        where = (leads, L, B, mode, si, name, grid, wp, th, lds)
                        assert name in INSTANCES, where
                        lout = L >> rows[si][18]
                        lin = L if rows[si][9] == -2 else L >> rows[rows[si][9]][18]
                        special = "_t<" in name
                        assert special == (lin % 4 == 0 and lout % 4 == 0), where
                        assert name.startswith("k_unet_bwd" if mode == "bwd" else "k_unet_fwd"), where
                        assert th == (512 if special else 256) and 1 <= wp <= (2 if mode == "bwd" else 4), where
                        assert 0 < lds <= 160 * 1024 and (lds <= 80 * 1024 or not special or wp == 1), where
                        assert 1 <= grid <= min(B, GRID_CAP), where
                        # a workgroup loops over passes of wp windows: no pass is empty for every workgroup, none is left out
                        passes = -(-B // (grid * wp))
                        assert passes >= 1 and (passes - 1) * grid * wp < B <= passes * grid * wp, where
                        assert special or wp == 1, where
                        if special and mode != "bwd":          # (the backward keeps min(B, 512) workgroups: the fold's rows)
                            assert (grid - 1) * wp < B, where
                        if mode == "bwd":
                            bwd_grids.add(grid)
                        assert fold == (1 if L % 64 == 0 else 0), where
                # the fold sums one scratch row per workgroup of a backward stage: the same rows for all 11 stages
                assert bwd_grids == {min(B, GRID_CAP)}, (leads, L, B, bwd_grids)


def test_query_refuses_what_a_model_refuses():
    lib = _lib.lib()
    for (leads, L, B, si), text in [((3, 512, 4, 0), b"leads must be 1 or 2 (got 3)"), ((2, 500, 4, 0), b"U-Net: L must be a multiple of 16 and <= 2048 (got 500)"),
                                    ((2, 2064, 4, 0), b"U-Net: L must be a multiple of 16 and <= 2048 (got 2064)"), ((2, 512, 0, 0), b"max_batch must be positive"),
                                    ((2, 512, 4, 11), b"U-Net stage 11 outside [0, 10]"), ((2, 512, 4, -2), b"U-Net stage -2 outside [0, 10]")]:
        assert lib.ral_unet_stage_plan(0, leads, L, B, 1, si, 1, None, 0, None, None, None, None, None, None) != 0
        assert lib.ral_last_error() == text
        cfg = _lib.make_config("unet", leads, L, B, 1)
        if si == 0:
            assert lib.ral_workspace_bytes(C.byref(cfg)) < 0 and lib.ral_last_error() == text      # the same text as the model's
    assert lib.ral_unet_stage_plan(0, 2, 512, 4, 1, 0, 1, None, 0, None, None, None, None, None, None) == 0   # every out-pointer may be NULL


# ---- the ledger
def train_step_cases():
    import test_gpu_unet as G
    cases = [m for m in G.test_unet_train_step_matches_oracle.pytestmark if m.name == "parametrize"][0].args[1]
    return list(dict.fromkeys(c.values[0] for c in cases))             # (shape, input seed, yardstick seeds): the shapes


def launched_by(leads, L, B):
    """the instances test_unet_train_step_matches_oracle launches at a case: a train step, then an eval forward (fused where the
    model fuses it - the default - else stage by stage)"""
    got = {query(mode, leads, L, B, si)[0] for mode in ("train", "bwd") for si in range(11)}
    fused = query("eval", leads, L, B, -1)
    got |= {fused[0]} if fused[6] else {query("eval", leads, L, B, si)[0] for si in range(11)}
    return got


def uncovered(cases):
    """[(instance, witness)]: instances no case launches, each with the smallest (leads, L) that would"""
    covered = set().union(*[launched_by(*c) for c in cases]) if cases else set()
    witness = {}
    for L in range(16, 2049, 16):
        for leads in (1, 2):
            for name in launched_by(leads, L, 2):
                witness.setdefault(name, "leads=%d L=%d" % (leads, L))
    assert set(witness) == set(INSTANCES)          # a model reaches every instance
    return [(n, witness[n]) for n in sorted(INSTANCES) if n not in covered]


def test_the_oracle_cases_launch_every_instance():
    """on failure: each instance no case of test_unet_train_step_matches_oracle launches, with a configuration that does -
    add a case for it there (B <= 5)"""
    cases = train_step_cases()
    missing = uncovered(cases)
    assert not missing, "\n".join(["no oracle case launches:"] + ["  %s   e.g. %s" % m for m in missing])
    # the staged eval forward is compared too: some case has a length the fused kernel does not take but the specialised kernels do
    assert any(not query("eval", le, L, B, -1)[6] and L % 64 == 0 for le, L, B in cases)


def test_the_ledger_is_sensitive():
    """without the L = 48 case exactly the two generic kernels are uncovered; without the one-lead case its four instances"""
    cases = train_step_cases()
    assert [n for n, _ in uncovered([c for c in cases if c[1] != 48])] == ["k_unet_bwd", "k_unet_fwd"]
    assert [n for n, _ in uncovered([c for c in cases if c[0] != 1])] == ["k_unet_bwd_t<1, 4, 3, 0>", "k_unet_bwd_t<4, 1, 4, 2>", "k_unet_fwd_t<1, 4, 3, 0>",
                                                                           "k_unet_fwd_t<4, 1, 4, 2>", "k_unet_infer<1>"]
