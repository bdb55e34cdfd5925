"""The ledger of the Linear-layer kernel instances (BLOCK_KERNELS, csrc/ral_block_plan.hpp), on the CPU: which of them a model can
launch, and which GPU test compares what each computes with the fp64 oracle or the reference goldens.

tests/test_block_plan_cpu.py shows that the plan chooses every instance at some point of the legal (C, N) space.  That says
nothing about whether a model has such a point - the levels of a model are (8 << l, Lp >> l) with Lp a multiple of 256 - nor
about whether a GPU test has ever run the instance.  Here, with `ral_block_plan` alone (a process per option string: the switches
latch at their first read):

  reachable  the instances some model launches: window lengths 16 .. 1024 in steps of 16 (a padded length forces f16_split 0 and
             gives NE = L >> l), levels 0 .. 4, training and eval, f16_split in {0, 32, 64, 128} x narrow_f16 in {0, 1}, a second
             output at level 4 only (block 9), every documented value of the four switches (one switch off its default at a time);
  covered    the instances launched by the configurations the oracle-comparing GPU tests run, read from the tests' own
             parametrize marks (TESTS below says per test function what it runs - nothing else is kept by hand).

reachable is every instance but the four of NO_MODEL_HAS, covered equals reachable, and every forward instance an eval-mode model
launches is covered by an eval-mode comparison.  Tests that compare one path of the library with another do not count."""
import inspect
import json
import os
import re
import subprocess
import sys

import pytest

import test_block_plan_cpu as T

ROOT = T.ROOT

# documented values of the four switches (csrc/ral_block_plan.hip); the last of each is the default
DOCUMENTED = {"mlp_fwd_w": (0, 1, 2, 3), "mlp_bwd_w": (0, 1, 2, 3), "mlp_bwd_w_f16": (0, 1), "fuse_dw": (0, 8, 16, 32)}
SWITCH_STRINGS = [""] + ["%s=%d" % (k, v) for k, values in DOCUMENTED.items() for v in values[:-1]]

# instance -> the (C, N) that choose it, and why no level of a model is one of them.  (Levels: C = 8 has N = Lp in {256, 512, 768,
# 1024}, C = 16 has N = Lp / 2 in {128, 256, 384, 512}.  The plan-space sweep of tests/test_block_plan_cpu.py still reaches
# them and the plan aborts on a missing instance, so they stay built.)
NO_MODEL_HAS = {
    "k_mlp_fwd<16, 2>": ("C = 16, N = 192 .. 240", "two hidden chunks fit between N = 176 and 256 only; level 1 has N = 128, then 256 (four chunks)"),
    "k_mlp_bwd<8, 2>": ("C = 8, N = 352 .. 480", "level 0 has N = 256 (one chunk), then 512 (four)"),
    "k_mlp_bwd<16, 2>": ("C = 16, N = 176 .. 240", "level 1 has N = 128 (one chunk), then 256 (four)"),
    "k_mlp_bwd_s<8, 1>": ("C = 8, N = 128", "one token tile per wave needs a window of 128 tokens at level 0; the shortest has 256 slots"),
}

# what each oracle-comparing GPU test runs.  modes: 1 training (a whole train step), 0 eval (forward); f16_split / narrow_f16: the
# model's defaults unless the test's cases carry their own; under: the option strings of the processes it runs in; lengths: where
# its window lengths come from.
TESTS = {
    "test_train_step_matches_oracle": dict(ref="fp64", modes=(1,), f16_split=64, narrow_f16=1,
                                           under='"" and each string of test_narrow_level_mlp_forward_kernel_choices', lengths="its mark"),
    "test_window_lengths_that_are_multiples_of_16_match_oracle": dict(ref="fp64", modes=(1,), f16_split=64, narrow_f16=1, under='""', lengths="its mark"),
    "test_against_reference_golden": dict(ref="goldens", modes=(1, 0), f16_split=64, narrow_f16=1, under='""', lengths="its mark"),
    "_scaled_parity": dict(ref="fp64", modes=(1,), f16_split=0, narrow_f16=1, under='""', lengths="512, in its body"),   # the f16_split=0 leg
    "test_block_instances_match_oracle": dict(ref="fp64", modes=(1, 0), f16_split="its mark", narrow_f16=1,
                                              under='"" and the strings of test_block_instances_under_latched_switches that name the case',
                                              lengths="its mark"),
}


def covering_runs(with_instance_file=True):
    """[(test, option string, L, mode, f16_split, narrow_f16)] of the tests above, from their parametrize marks"""
    import test_gpu_block_instances as I
    import test_gpu_configs as G
    import test_gpu_parity as P
    runs = []

    def add(test, opts, Lw, f16_split=None):
        t = TESTS[test]
        runs.extend((test, opts, Lw, mode, t["f16_split"] if f16_split is None else f16_split, t["narrow_f16"]) for mode in t["modes"])

    strip_strings = T.parametrize_args(G.test_narrow_level_mlp_forward_kernel_choices)
    assert "train_step_matches_oracle" in inspect.getsource(G.test_narrow_level_mlp_forward_kernel_choices)
    for _, _, Lw, _ in T.parametrize_args(P.test_train_step_matches_oracle):
        for opts in [""] + strip_strings:
            add("test_train_step_matches_oracle", opts, Lw)
    for _, _, Lw, _ in T.parametrize_args(P.test_window_lengths_that_are_multiples_of_16_match_oracle):
        add("test_window_lengths_that_are_multiples_of_16_match_oracle", "", Lw)
    for _, _, Lw in T.parametrize_args(P.test_against_reference_golden):
        add("test_against_reference_golden", "", Lw)
    assert "L=512" in inspect.getsource(G._scaled_parity) and "f16_split=0" in inspect.getsource(G)
    add("_scaled_parity", "", 512)
    if with_instance_file:
        cases = {c.id: c.values for c in T.parametrize_args(I.test_block_instances_match_oracle)}
        assert I.NARROW_F16 == TESTS["test_block_instances_match_oracle"]["narrow_f16"]
        for values in cases.values():
            add("test_block_instances_match_oracle", "", values[1], values[3])
        for opts, ids in T.parametrize_args(I.test_block_instances_under_latched_switches):
            for i in ids:
                add("test_block_instances_match_oracle", T.switch_part(opts), cases[i][1], cases[i][3])
    return runs


_CHILD = r"""
import json, sys
sys.path.insert(0, %(tests)r)
import test_block_plan_cpu as T
from ecg_denoise_amd import _lib
_lib.apply_options(%(opts)r)
L = _lib.lib()
names, rows = {}, []
for Lw in range(16, 1025, 16):
    for fs in ((0, 32, 64, 128) if Lw %% 256 == 0 else (0,)):
        for nar in (0, 1):
            for tr in (1, 0):
                for l, Cw, N, NE, so, f in T.model_points(Lw, fs):
                    got = [T.plan(i, Cw, N, NE, tr, so, 1, f, nar, L)[0] for i in (range(8) if tr else (0, 1))]
                    rows.append([Lw, l, tr, fs, nar, [names.setdefault(n, len(names)) for n in got if n]])
print(json.dumps({"names": list(names), "rows": rows}))
"""


def _child(opts):
    code = _CHILD % {"tests": os.path.join(ROOT, "tests"), "opts": opts}
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    launched = {}          # (L, mode, f16_split, narrow_f16) -> {(instance, level)}
    for Lw, l, tr, fs, nar, idx in out["rows"]:
        launched.setdefault((Lw, tr, fs, nar), set()).update((out["names"][i], l) for i in idx)
    return launched


@pytest.fixture(scope="module")
def launched():
    """option string -> what every model launches in a fresh process with these switches"""
    strings = list(dict.fromkeys(SWITCH_STRINGS + [opts for _, opts, *_ in covering_runs()]))
    return {opts: _child(opts) for opts in strings}


def every_instance():
    hpp = open(os.path.join(ROOT, "ecg_denoise_amd", "csrc", "ral_block_plan.hpp")).read()
    return set(re.findall(r'^\s*X\(\w+, "([^"]+)"\)', hpp, flags=re.M))


def reachable_with_witness(launched):
    """({instance: witness}, {forward instance an eval-mode model launches: witness}); a witness is the first option string, L,
    level, mode, f16_split and narrow_f16 that launch the instance"""
    first, first_eval = {}, {}
    for opts in SWITCH_STRINGS:
        for (Lw, tr, fs, nar), got in sorted(launched[opts].items()):
            for name, l in sorted(got):
                witness = "opts=%r L=%d level=%d mode=%s f16_split=%d narrow_f16=%d" % (opts, Lw, l, "training" if tr else "eval", fs, nar)
                first.setdefault(name, witness)
                if not tr:
                    first_eval.setdefault(name, witness)
    return first, first_eval


def covered_by(launched, runs):
    """({instances}, {forward instances covered in eval mode}) of the runs"""
    every, in_eval = set(), set()
    for _, opts, Lw, mode, fs, nar in runs:
        got = {name for name, _ in launched[opts][(Lw, mode, fs if Lw % 256 == 0 else 0, nar)]}
        every |= got
        if not mode:
            in_eval |= got
    return every, in_eval


def uncovered(launched, runs):
    """[(instance, witness)] that a model can launch and no run compares; [(forward instance, witness)] not compared in eval mode"""
    first, first_eval = reachable_with_witness(launched)
    every, in_eval = covered_by(launched, runs)
    return [(n, w) for n, w in sorted(first.items()) if n not in every], [(n, w) for n, w in sorted(first_eval.items()) if n not in in_eval]


def test_the_ledger_strings_are_pinned_and_documented(launched):
    """every option string of the ledger has a written-out table in tests/test_block_plan_cpu.py, and the switch values are the
    ones csrc/ral_block_plan.hip documents"""
    assert set(launched) <= set(T.EXPECTED), sorted(set(launched) - set(T.EXPECTED))
    hip = open(os.path.join(ROOT, "ecg_denoise_amd", "csrc", "ral_block_plan.hip")).read()
    assert {m.lower(): int(d) for m, d in re.findall(r'^BLOCK_SWITCH\(\w+, "(\w+)", (\d+)\)', hip, flags=re.M)} == {k: v[-1] for k, v in DOCUMENTED.items()}


def test_a_model_reaches_every_instance_but_four(launched):
    reachable = set(reachable_with_witness(launched)[0])
    every = every_instance()
    assert len(every) >= 100 and set(NO_MODEL_HAS) <= every
    assert every - reachable == set(NO_MODEL_HAS), (sorted(every - reachable), sorted(reachable - every))
    assert reachable == every - set(NO_MODEL_HAS)


def test_every_reachable_instance_is_compared_with_the_oracle(launched):
    """covered == reachable; a forward instance an eval-mode model launches is compared in eval mode.  On failure: each instance
    with one configuration that launches it - add a case for it to tests/test_gpu_block_instances.py."""
    runs = covering_runs()
    missing, missing_eval = uncovered(launched, runs)
    every, in_eval = covered_by(launched, runs)
    reachable = set(reachable_with_witness(launched)[0])
    msg = "\n".join(["no GPU test compares these with the oracle:"] + ["  %s   e.g. %s" % m for m in missing]
                    + ["never compared in eval mode:"] + ["  %s   e.g. %s" % m for m in missing_eval])
    assert not missing and not missing_eval, msg
    assert every == reachable, sorted(every - reachable)          # (a test runs nothing the reachable set does not have)
    assert {t for t, *_ in runs} == set(TESTS)


def test_without_the_instance_file_the_ledger_names_what_its_cases_exist_for(launched):
    """the ledger is sensitive: without the cases of tests/test_gpu_block_instances.py exactly the instances those cases say
    they exist for are uncovered"""
    import test_gpu_block_instances as I
    missing, missing_eval = uncovered(launched, covering_runs(with_instance_file=False))
    declared = {n for c in T.parametrize_args(I.test_block_instances_match_oracle) for names in c.values[4].values() for n in names}
    assert missing and {n for n, _ in missing + missing_eval} == declared, (missing, missing_eval, sorted(declared))
