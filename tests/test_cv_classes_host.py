"""The census of the cross-validation class cases (CPU; g++ builds tests/cv_plan_check.cpp and
tests/cvpath_plan_check.cpp): every row of tests/cv_class_cases.py is held against the host plan the
library launches from (bmc_cv_plan.h, bmc_cvpath_plan.h), so the table keeps reaching what its
docstring says when a constant of the plan moves, and a row cannot leave without a failure here."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cv_class_cases as CC
import cv_reference as CV

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pybmc_amd", "csrc")

# the rows the table must have: taking one out fails test_the_table_is_whole and the test of its class
ROWS = tuple(f"width_{k}" for k in (15, 16, 31, 32, 47, 48, 63)) + \
    ("nt4_tight", "chunk_edges", "loo", "max_folds", "gather_wrap", "unrotate_wrap")
PATH_ROWS = ("tile_fill", "split_classes")


def _constant(name, header="bmc_cv_plan.h"):
    text = open(os.path.join(CSRC, header)).read()
    return int(re.search(name + r" = (\d+);", text).group(1))


MAX_LAUNCH = _constant("CV_MAX_CHAINS_PER_LAUNCH")
GRAM_CHUNK, RSS_CHUNK, ROW_PAD = _constant("CV_GRAM_CHUNK"), _constant("CV_RSS_CHUNK"), _constant("CV_ROW_PAD")
STRIDE = _constant("CV_STRIDE_THREADS") * _constant("CV_STRIDE_BLOCKS")   # elements of one grid-stride trip


def _build(tmp, source):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is required")
    out = tmp / source[:-4]
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, source), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(out)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("cv_classes"), "cv_plan_check.cpp")


@pytest.fixture(scope="module")
def path_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("cv_classes_path"), "cvpath_plan_check.cpp")


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip()


def widths(exe):
    """k -> (ldz, tiles, kmax) for k = 1 .. 64, from the header"""
    table = {}
    for line in run(exe, "widths").splitlines():
        k, ldz, tiles, kmax = (int(v) for v in line.split())
        table[k] = (ldz, tiles, kmax)
    assert sorted(table) == list(range(1, 65))
    return table


def chunks(exe, folds, F):
    """(n_pad, rows of the Gram chunks per fold, rows of the rss chunks per fold)"""
    n_pad, gram, rss = run(exe, "chunks", F, *folds.tolist()).split(" | ")

    def per_fold(text):
        items, off = text.split("/")
        rows = [int(v.split("+")[1]) for v in items.split(",")]
        off = [int(v) for v in off.split(",")]
        return [rows[off[f]:off[f + 1]] for f in range(F)]
    return int(n_pad), per_fold(gram), per_fold(rss)


def test_the_table_is_whole():
    assert tuple(CC.CASES) == ROWS and tuple(CC.PATH_CASES) == PATH_ROWS
    assert set(CC.PICKS) <= set(ROWS)
    for k in CC.WIDTHS:
        n, kk, spec, C, T, snr, scale = CC.CASES[f"width_{k}"]
        assert (n, kk, spec, C, T) == (6 * k + 1, k, 3, 1, 65)
    assert CC.T_EDGES == (1, 63, 64, 65, 128) and CC.T_EDGE_CASE in CV.CASES
    for name in ROWS:
        A, y, prior, folds, F, C, T = CC.case(name)
        n, k = CC.CASES[name][:2]
        assert A.shape == (n, k) and y.shape == (n,) and folds.shape == (n,)
        assert np.array_equal(np.unique(folds), np.arange(F))


def direct_widths():
    """The widths at which some GPU test calls kfold_cv on its own: this table, cv_reference.CASES
    and the single calls of test_cvpath_gpu's `edges`."""
    import test_cvpath_gpu as P
    ks = {CC.CASES[name][1] for name in CC.CASES} | {v[1] for v in CV.CASES.values()}
    return ks | set(P.make_case("edges")[6])


def test_every_width_class_is_reached_on_both_sides_of_its_edge(exe):
    table = widths(exe)
    pairs = {}
    for k, (ldz, tiles, kmax) in table.items():
        assert ldz == 16 * tiles and ldz >= k + 1 > ldz - 16
        pairs.setdefault((tiles, kmax), []).append(k)
    assert sorted(pairs) == [(1, 8), (1, 16), (2, 16), (2, 32), (3, 32), (3, 64), (4, 64), (5, 64)]
    reached = direct_widths()
    for pair, ks in pairs.items():
        assert reached & set(ks), f"no GPU case at (tiles, KMAX) = {pair}"
        # ... and at the first and the last width of the pair
        assert min(ks) in reached and max(ks) in reached, f"{pair}: widths {min(ks)} and {max(ks)}"
    # the widths at which [A | y] fills its last tile exactly are rows of THIS table
    fill = [k for k, (ldz, _, _) in table.items() if ldz == k + 1 and k < 64]
    assert tuple(fill) == CC.EXACT_FILL and all(f"width_{k}" in CC.CASES for k in fill)
    # cv_fold_gram_kernel<4>
    assert table[48][1] == 4 and table[63][1] == 4 and "width_48" in CC.CASES and "width_63" in CC.CASES
    # the tight fit at 4 tiles / KMAX 64, where the existing one is at 2 / 32
    assert table[CC.CASES["nt4_tight"][1]][1:] == (4, 64) and table[CV.CASES["tight_scaled"][1]][1:] == (2, 32)
    assert CC.CASES["nt4_tight"][5:] == (CV.CASES["tight_scaled"][4], CV.SCALE["tight_scaled"])


def test_chunk_edges_meets_every_edge_of_both_chunk_tables(exe):
    A, y, prior, folds, F, C, T = CC.case("chunk_edges")
    assert np.array_equal(np.bincount(folds), CC.CHUNK_SIZES)
    G, R = GRAM_CHUNK, RSS_CHUNK
    assert CC.CHUNK_SIZES == (1, 2, 3, R - 1, R, R + 1, G - 1, G, G + 1) and (G, R, ROW_PAD) == (512, 64, 4)
    n_pad, gram, rss = chunks(exe, folds, F)
    assert gram == [[4], [4], [4], [64], [64], [68], [512], [512], [512, 4]]
    assert rss == [[1], [2], [3], [63], [64], [64, 1], [64] * 7 + [63], [64] * 8, [64] * 8 + [1]]
    assert n_pad == sum(sum(g) for g in gram) == 1748
    # row padding of 3, 2, 1 and 0 rows all occur
    assert {sum(g) - s for g, s in zip(gram, CC.CHUNK_SIZES)} == {0, 1, 2, 3}


def test_loo_and_max_folds(exe):
    A, y, prior, folds, F, C, T = CC.case("loo")
    n = len(y)
    assert F == n and np.array_equal(np.sort(folds), np.arange(n))        # a permutation
    n_pad, gram, rss = chunks(exe, folds, F)
    assert n_pad == 4 * n and gram == [[4]] * n and rss == [[1]] * n
    assert T == 64 and tuple(divmod(g, C) for g in CC.PICKS["loo"]) == ((0, 0), (0, 1), (64, 0), (64, 1), (129, 0), (129, 1))

    A, y, prior, folds, F, C, T = CC.case("max_folds")
    assert F == _constant("CV_MAX_FOLDS") == len(y) and F * C == MAX_LAUNCH
    head, tail = run(exe, "batches", F, C, A.shape[1], T, 0, 1, 1 << 60).split("|")
    assert tail.split() == [f"0-{F}:0+{MAX_LAUNCH}"]                       # one launch, exactly full
    assert (2 * F + 63) // 64 == 32                                      # gridDim.y of cv_block_rss_kernel
    assert CC.PICKS["max_folds"] == (0, F * C // 2 - 1, F * C // 2, F * C - 1)


def elements(exe, A, folds, F, C, T, table):
    """(gathered elements, un-rotated elements) of a kfold_cv call in one batch, burn 0, thin 1"""
    k = A.shape[1]
    n_pad = chunks(exe, folds, F)[0]
    return n_pad * table[k][0], F * C * T * (k + 1)


def test_the_wrap_cases_make_a_second_trip_and_nothing_else_did(exe):
    table = widths(exe)
    assert STRIDE == 2097152
    A, y, prior, folds, F, C, T = CC.case("gather_wrap")
    gathered, unrotated = elements(exe, A, folds, F, C, T, table)
    assert gathered == 2160000 > STRIDE > unrotated
    behind = CC.rows_behind(folds, F, A.shape[1], STRIDE)
    assert len(behind) == (gathered - STRIDE + 79) // 80 and (folds[behind] == 1).all()
    A, y, prior, folds, F, C, T = CC.case("unrotate_wrap")
    gathered, unrotated = elements(exe, A, folds, F, C, T, table)
    assert unrotated == 2496000 > STRIDE > gathered
    per_chain = T * (A.shape[1] + 1)
    assert STRIDE // per_chain == 107 and STRIDE % per_chain                # chain 107 straddles the wrap
    assert CC.PICKS["unrotate_wrap"] == (0, 107, 108, F * C - 1)
    # the largest launches of the suite before these cases stay inside one trip
    A, y, prior, folds, F, C = CV.case("wide")
    gathered, unrotated = elements(exe, A, folds, F, C, CV.T, table)
    assert gathered < STRIDE and unrotated < STRIDE
    assert 2100 * 20 * 3 < STRIDE and (200 + 3 * 30) * 16 < STRIDE          # test_cv_gpu.py::test_launch_split
    for name in CC.CASES:
        if name not in ("gather_wrap", "unrotate_wrap"):
            A, y, prior, folds, F, C, T = CC.case(name)
            assert max(elements(exe, A, folds, F, C, T, table)) < STRIDE, name


def test_the_path_cases(exe, path_exe):
    table = widths(exe)
    n, k, F, C, T, comps, picks = CC.PATH_CASES["tile_fill"]
    assert comps == CC.WIDTHS and k == max(comps) and table[k][1] == 4       # the path gathers at 4 tiles
    assert [table[c][1] for c in comps] == [1, 2, 2, 3, 3, 4, 4]             # ... the single calls here
    n, k, _, C, T, comps, picks = CC.PATH_CASES["split_classes"]
    F = CC.SPLIT_FOLDS
    assert [table[c][2] for c in comps] == [8, 16] and F * C == 2100
    kept, per, tail = run(path_exe, "plan", F, C, T, 0, 1, 1 << 60, *comps).split("|")
    launches = tail.split()[0].split(":")[1].split(",")
    assert len(tail.split()) == 1                                           # one batch
    assert launches == [f"16@2100+{MAX_LAUNCH}", "16@4148+52", f"8@0+{MAX_LAUNCH}", "8@2048+52"]
    assert picks == (0, 2047, 2048, 2099, 2100, 4147, 4148, 4199)
