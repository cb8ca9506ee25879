"""plan_predict_orderstat (pybmc_amd/csrc/bmc_plan.h) on the CPU: g++ builds
tests/predict_plan_check.cpp, which includes the header the library is built from.  The route of
the predictive leg's order statistics (sort or selection, which instantiation, grid, block, LDS),
and the guarantee that the shared case list (tests/predict_cases.py) reaches every class of it with
rows of every branch of the selection -- conditions on the plan and on the inputs, checked without
the library."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import predict_cases as PC
import predict_reference as PR
from pybmc_amd._lib import order_stat_plan

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is required")
    exe = tmp_path_factory.mktemp("predict_plan") / "predict_plan_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                        os.path.join(HERE, "predict_plan_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def _kv(exe, *args):
    r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return dict((kv.split("=")[0], int(kv.split("=")[1])) for kv in r.stdout.split())


def plan(exe, S, n_q=6, n_cov=21, M=70):
    return _kv(exe, "plan", S, n_q, n_cov, M)


def case_plan(exe, case):
    return plan(exe, case.S, len(case.q), 0 if case.cov is None else len(case.cov), case.M)


def test_constants_of_the_mirror(plan_exe):
    c = _kv(plan_exe, "constants")
    assert (c["SEL_BINS"], c["SEL_CAP"], c["SEL_THREADS"]) == (PR.SEL_BINS, PR.SEL_CAP, PR.SEL_THREADS)
    assert (c["MAX_DRAWS"], c["MAX_Q"], c["MAX_COV"]) == (16384, 64, 64)
    assert (c["SELECT_MIN_DRAWS"], c["SELECT_MAX_RANKS"]) == (2048, 128)
    assert (c["MAX_BLOCKS"], c["FALLBACK_BLOCKS"]) == (2048, 256)


# S -> (nsort, sort_threads): both sides of every power of two, the 128-thread floor (nsort <= 256)
# and the 1024-thread cap (nsort >= 2048)
@pytest.mark.parametrize("S,nsort,threads", [
    (1, 64, 128), (64, 64, 128), (65, 128, 128), (128, 128, 128), (129, 256, 128), (256, 256, 128),
    (257, 512, 256), (512, 512, 256), (513, 1024, 512), (1024, 1024, 512), (1025, 2048, 1024),
    (2047, 2048, 1024)])
def test_named_sort_shapes(plan_exe, S, nsort, threads):
    p = plan(plan_exe, S)
    assert p["ok"] == 1 and p["launch"] == 1 and p["select"] == 0
    assert (p["vpt"], p["nsort"], p["sort_threads"]) == (0, nsort, threads)
    assert (p["blocks_select"], p["blocks_sort"]) == (0, 70)
    assert (p["lds_select"], p["lds_sort"]) == (0, nsort * 8)


# every 512 * 4 j and the value after it
@pytest.mark.parametrize("S,vpt,nsort", [
    (2048, 8, 2048), (2049, 8, 4096), (4096, 8, 4096), (4097, 12, 8192), (6144, 12, 8192),
    (6145, 16, 8192), (8192, 16, 8192), (8193, 20, 16384), (10240, 20, 16384), (10241, 24, 16384),
    (12288, 24, 16384), (12289, 28, 16384), (14336, 28, 16384), (14337, 32, 16384),
    (16384, 32, 16384)])
def test_named_select_shapes(plan_exe, S, vpt, nsort):
    p = plan(plan_exe, S)
    assert p["ok"] == 1 and p["launch"] == 1 and p["select"] == 1
    assert (p["vpt"], p["nsort"], p["sort_threads"]) == (vpt, nsort, 1024)
    assert (p["blocks_select"], p["blocks_sort"]) == (70, 70)
    n_t = 2 * 6 + 2 * 21
    assert p["lds_select"] == 4096 * 8 + 128 + 64 + 2048 + 16 * n_t + 16 + 512 * n_t
    assert p["lds_sort"] == nsort * 8


def test_requested_ranks_boundary(plan_exe):
    """128 requested ranks still select; 130 take the sort, as do the request limits."""
    a, b = plan(plan_exe, 4096, 43, 21), plan(plan_exe, 4096, 44, 21)
    assert (a["select"], a["vpt"]) == (1, 8) and (b["select"], b["vpt"], b["lds_select"]) == (0, 0, 0)
    assert a["lds_select"] == 4096 * 8 + 128 + 64 + 2048 + 16 * 128 + 16 + 512 * 128 <= 160 * 1024
    assert b["nsort"] == 4096 and b["sort_threads"] == 1024
    c = plan(plan_exe, 64, 64, 64)
    assert (c["select"], c["nsort"], c["sort_threads"]) == (0, 64, 128)   # threads 64..127: 64 intervals
    assert plan(plan_exe, 10000, 64, 64)["select"] == 0
    assert plan(plan_exe, 16384, 0, 64)["select"] == 1 and plan(plan_exe, 16384, 64, 0)["select"] == 1


def test_point_loops(plan_exe):
    """At most 2048 workgroups walk the points; the sort behind the selection gets at most 256."""
    for M, first, second in [(1, 1, 1), (255, 255, 255), (256, 256, 256), (257, 257, 256),
                             (2048, 2048, 256), (2100, 2048, 256), (50000, 2048, 256)]:
        p = plan(plan_exe, 2048, M=M)
        assert (p["blocks_select"], p["blocks_sort"]) == (first, second)
        p = plan(plan_exe, 2047, M=M)
        assert (p["blocks_select"], p["blocks_sort"]) == (0, first)


def test_nothing_asked_launches_nothing(plan_exe):
    p = plan(plan_exe, 10000, 0, 0)
    assert p["ok"] == 1 and p["launch"] == 0


@pytest.mark.parametrize("S,n_q,n_cov,M", [(0, 6, 21, 70), (16385, 6, 21, 70), (100, 65, 0, 70),
                                           (100, 0, 65, 70), (100, -1, 0, 70), (100, 6, 21, 0)])
def test_refusals(plan_exe, S, n_q, n_cov, M):
    p = plan(plan_exe, S, n_q, n_cov, M)
    assert p["ok"] == 0 and p["launch"] == 0 and p["blocks_sort"] == 0 and p["lds_sort"] == 0


@pytest.fixture(scope="module")
def sweep_classes(plan_exe):
    r = subprocess.run([plan_exe, "sweep"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    lines = r.stdout.strip().splitlines()
    plans, fails = lines[-1].split()[-2:]
    assert int(plans) == 16386 * 14 * 10 and int(fails) == 0
    return {tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("class ")}


def test_sweep(sweep_classes):
    """Every S x a few requests x a few point counts meets the invariants, and the classes are
    the nine sorts and the eight (draws per thread, fallback sort) pairs of the selection."""
    sorts = {(0, 0, n) for n in (64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384)}
    selects = {(1, 8, 2048), (1, 8, 4096), (1, 12, 8192), (1, 16, 8192), (1, 20, 16384),
               (1, 24, 16384), (1, 28, 16384), (1, 32, 16384)}
    assert sweep_classes == sorts | selects


# ---- the case list ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def case_routes():
    """name -> the selection's branch for every point of the case (S >= 2048 only)."""
    out = {}
    for case in PC.CASES:
        if case.S < 2048:
            continue
        noise = PC.case_inputs(case)["noise"]
        ranks = PR.requested_ranks(case.S, case.q, case.cov)
        out[case.name] = [PR.selection_route(noise[:, p], ranks) for p in range(case.M)]
    return out


def test_case_list_reaches_every_class(plan_exe, sweep_classes, case_routes):
    """The coverage guarantee: every class the plan can produce is launched by a case -- each
    draws-per-thread class by the selection, each sort size as the primary route, and the sort
    sizes 2048 .. 16384 also as the second pass behind a selection that hands points back."""
    seen, primary, fallback = set(), set(), set()
    for case in PC.CASES:
        p = case_plan(plan_exe, case)
        assert p["ok"] == 1 and p["launch"] == 1
        seen.add((p["select"], p["vpt"], p["nsort"]))
        if p["select"]:
            if "fallback" in case_routes[case.name] or "unusable" in case_routes[case.name]:
                fallback.add(p["nsort"])
        else:
            primary.add(p["nsort"])
    assert seen == sweep_classes
    assert {v for s, v, _ in seen if s} == {8, 12, 16, 20, 24, 28, 32}
    assert primary == {64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384}
    assert fallback >= {2048, 4096, 8192, 16384}
    # the block-size floor and cap, the request limits and both point loops are crossed
    plans = {c.name: case_plan(plan_exe, c) for c in PC.CASES}
    assert {p["sort_threads"] for p in plans.values()} == {128, 256, 512, 1024}
    assert plans["S64-q64-cov64"]["sort_threads"] == 128
    assert plans["S64-M2100"]["blocks_sort"] == 2048 < 2100
    assert (plans["S2048-M2100"]["blocks_select"], plans["S2048-M2100"]["blocks_sort"]) == (2048, 256)
    assert sum(r != "select" and r != "flat" for r in case_routes["S2048-M2100"]) > 256


def test_every_selection_case_mixes_the_routes(plan_exe, case_routes):
    """A condition on the inputs: each call the selection serves holds rows of all four branches
    (so fail_points / fail_count carry some points and not others), and every row kind takes the
    branch it was built for -- the +-1e300 row is handed back, the 8-fold ties are resolved."""
    n = 0
    for case in PC.CASES:
        if case.S < 2048:
            continue
        routes = case_routes[case.name]
        assert set(routes) == {"flat", "unusable", "select", "fallback"}, case.name
        if case_plan(plan_exe, case)["select"]:
            n += 1
        for p, r in enumerate(routes):
            assert r == PC.EXPECTED_ROUTE[PC.row_kind(p)], (case.name, p, PC.row_kind(p), r)
    assert n >= len(PC.S_SELECT) + 3


def test_truth_values_sit_on_and_beside_the_bounds():
    """Per call: a truth equal to a lower bound's order statistic, one equal to an upper bound's,
    and one a single ulp outside each -- for a row the selection resolves and one it hands back."""
    for case in (c for c in PC.CASES if c.cov is not None and c.S >= 64):
        inp = PC.case_inputs(case)
        ranks = PR.requested_ranks(case.S, (), case.cov)
        c = len(case.cov) // 2 + 1
        lo, hi = ranks[2 * c], ranks[2 * c + 1]
        assert lo < hi
        srt = np.sort(inp["noise"], axis=0)
        t = inp["truth"]
        for base in (0, 2):
            assert t[base] == srt[lo, base] and t[base + 8] == srt[hi, base + 8]
            assert t[base + 16] > srt[hi, base + 16] and t[base + 16] == np.nextafter(srt[hi, base + 16], 9.0)
            assert t[base + 24] < srt[lo, base + 24] and t[base + 24] == np.nextafter(srt[lo, base + 24], -9.0)


def test_band_mirror_is_numpy_percentile():
    """What the GPU test demands bit for bit is attainable: sort + the kernels' interpolation
    with order_stat_plan's (index, weight) is np.percentile, for every request and row kind."""
    for case in PC.CASES:
        if not case.q or case.M > 70:
            continue
        noise = PC.case_inputs(case)["noise"]
        qi, qg = order_stat_plan(case.S, case.q)
        assert np.array_equal(PR.expected_bands(noise, qi, qg), np.percentile(noise, case.q, axis=0)), case.name


def test_reference_paths_agree():
    """The extended-precision reference and its exactly-rounded fallback agree far below the bar."""
    assert PR.longdouble_is_extended()
    rng = np.random.default_rng(5)
    M, Km, k, S = 5, 13, 7, 6
    preds, Vt = rng.standard_normal((M, Km)) + 3, rng.standard_normal((k, Km))
    theta = np.column_stack([rng.standard_normal((S, k)), rng.uniform(0.5, 1.5, S)])
    noise = rng.standard_normal((S, M))
    a, bar = PR.predictive_reference(preds, theta, Vt, noise)
    b, bar2 = PR.predictive_reference(preds, theta, Vt, noise, force_fsum=True)
    assert np.array_equal(bar, bar2) and (bar > 0).all()
    assert (np.abs(a - b) <= bar * 2.0 ** -8).all()
    # and float64 numpy itself meets the bar
    f = (theta[:, :-1] @ Vt + 1.0 / Km) @ preds.T + noise * theta[:, -1][:, None]
    assert (np.abs(f - a) <= bar).all()
