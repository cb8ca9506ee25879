"""tests/kernel_census.txt on the CPU: one line per compiled loop kernel, "name | recipe" (the
cheapest shape, chain count and tuning of the census grid whose plan launches it on a 256-CU
device) or "name | unreached".  The table is the planner's own output (launch_plan_check census);
test_kernel_census_gpu.py runs every recipe against the oracle.  A planner change that moves a
shape to another kernel fails here: measure it, then regenerate the table with

    g++ -std=c++17 -O2 -o /tmp/lpc tests/launch_plan_check.cpp && /tmp/lpc census > tests/kernel_census.txt
"""
import subprocess

import numpy as np
import pytest

import census_common as cc
from oracle import bmc_oracle as O

# Compiled loop kernels that no shape, chain count or tuning selects (DESIGN.md section 6 lists them
# and says why): the rows-per-lane-2 register kernels SINGLE and SMALLG, and the one-wave kernels on
# 2 / 4 or 8 waves whose panels a smaller wave count already holds within ONE_WAVE_MAX_FMAS, or
# whose rmax x kmax exceeds it.
UNREACHED = 69


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return cc.build_planner(tmp_path_factory.mktemp("planner"))


def test_every_compiled_kernel_appears_once(planner):
    names = subprocess.run([planner, "names"], check=True, capture_output=True, text=True).stdout.split("\n")
    names = [n for n in names if n]
    table = [name for name, _ in cc.read_table()]
    assert len(table) == len(set(table)) == len(names) == 405
    assert set(table) == set(names)


def test_every_recipe_still_launches_its_kernel(planner):
    plans = cc.replan(planner)
    moved = []
    for name, recipe in cc.read_table():
        if recipe is None:
            assert plans[name] is None
            continue
        launches, other = plans[name]
        if name not in [l[0] for l in launches]:
            moved.append((name, [l[0] for l in launches]))
        assert sum(l[2] for l in launches) == sum(l[2] for l in other) == recipe["chains"]
    assert not moved, moved


def test_the_table_is_the_census_and_the_unreached_are_counted(planner):
    """The committed table equals what the census search prints now (so the unreached set is what
    the search does not reach), and the number of unreached kernels is pinned."""
    out = subprocess.run([planner, "census"], check=True, capture_output=True, text=True).stdout
    with open(cc.TABLE) as f:
        pinned = f.read()
    got, want = out.splitlines(), pinned.splitlines()
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a == b
    unreached = [name for name, recipe in cc.read_table() if recipe is None]
    assert len(unreached) == UNREACHED
    # which they are: nothing else may join them unnoticed
    for name in unreached:
        fam, args = name.split("<")
        args = args.rstrip(">").split(", ")
        if fam in ("gibbs_loop_kernel", "simplex_loop_kernel"):
            assert args[1] == "2" and args[2] == "0", name            # rows per lane 2, registers
            assert args[5] == "true" or (fam == "gibbs_loop_kernel" and args[7] == "true"), name
        else:
            assert fam in ("gibbs_wave_kernel", "simplex_wave_kernel") and args[3] in ("4", "8", "true"), name


def test_recipes_are_problems_the_parity_tests_can_perturb():
    for name, r in cc.read_table():
        if r is None:
            continue
        assert r["k"] >= 2 and r["n"] >= 2 * r["k"] + 2, name
        if r["sampler"] == "simplex":
            assert r["chains"] == 1 and (not r["ow"] or r["k"] + 2 <= 64), name


def test_helper_loops_are_the_oracle():
    """census_common's chain loops with nothing perturbed are O.gibbs_replay / O.simplex_replay bit
    for bit, the slot colouring separates first, middle and last of every launch and bundle, and
    the perturbed oracles move a small problem's chain far beyond the f64 bar."""
    y, X, prior = cc.gibbs_problem(200, 3, 0)
    streams = cc.gibbs_streams(y, X, prior, 2, 40)
    ref, trace = cc.gibbs_chain(y, X, prior, *streams[0])
    want, wtrace = O.gibbs_replay(y, X, 40, prior, *streams[0], return_sigma2=True)
    assert np.array_equal(ref, want) and np.array_equal(trace, wtrace)
    for what, d in cc.gibbs_sensitivity(y, X, prior, streams, ref).items():
        assert d >= 100 * cc.F64_BAR, what
    assert cc.f32_rotation_error(*cc.gibbs_problem(200, 3, 1), *streams[0]) < cc.F32_CHAIN_CAP
    for launches in ([("a", 0, 64, 8)], [("a", 0, 16, 1)], [("a", 0, 56, 8), ("b", 56, 7, 1)], [("a", 0, 2, 2)],
                     [("a", 0, 8, 4), ("a", 8, 1, 1)], [("a", 0, 2048, 1), ("a", 2048, 952, 1)]):
        cc.assert_separated(cc.colour_slots(launches), launches)
    both = cc.colour_slots([("a", 0, 9, 1)], 5, [("b", 0, 8, 1), ("b", 8, 1, 1)])
    cc.assert_separated(both, [("a", 0, 9, 1)])
    cc.assert_separated(both, [("b", 0, 8, 1), ("b", 8, 1, 1)])
    c = cc.simplex_case(200, 2, 0, 1)        # (validates its loop against O.simplex_replay itself)
    assert 0 < c["acc_all"] < cc.BURN_SIMPLEX + cc.T_SIMPLEX and c["margin"] >= cc.MARGIN
    assert c["seed"] == cc.SIMPLEX_SEED
    for what, d in cc.simplex_sensitivity(c).items():
        assert d >= 100 * cc.F64_BAR, what
