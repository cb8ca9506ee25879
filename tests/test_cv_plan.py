"""CPU checks of the cross-validation plan (bmc_cv_plan.h; g++ builds tests/cv_plan_check.cpp): the
fold-ordered row layout, the split of F x C chains into batches and launches, the refusals, and the
declaration and binding of bmc_kfold_cv."""
import os
import re
import shutil
import subprocess

import pytest

from pybmc_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "pybmc_amd.h")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is required")
    out = tmp_path_factory.mktemp("cv_plan") / "cv_plan_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                        os.path.join(HERE, "cv_plan_check.cpp"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(out)


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip()


def ints(text):
    return [int(v) for v in text.split(",")]


def test_segments_of_unequal_folds(exe):
    # fold 0: rows 0, 3, 4, 6, 8 (five rows -> padded to 8); fold 1: row 2 alone; fold 2: rows 1, 5, 7
    labels = [0, 2, 1, 0, 0, 2, 0, 2, 0]
    off, cnt, src, gram, rss = run(exe, "segments", 3, *labels).split(" | ")
    assert ints(off) == [0, 8, 12, 16]                      # every fold starts on a multiple of 4
    assert ints(cnt) == [5, 1, 3]
    assert ints(src) == [0, 3, 4, 6, 8, -1, -1, -1,         # a stable permutation, zero rows behind
                         2, -1, -1, -1,
                         1, 5, 7, -1]
    assert gram == "0+8,8+4,12+4/0,1,2,3"                   # Gram chunks cover the padded rows
    assert rss == "0+5,8+1,12+3/0,1,2,3"                    # block-rss chunks the true rows


def test_long_folds_are_cut_into_chunks(exe):
    labels = [0] * 1100 + [1] * 70
    off, cnt, src, gram, rss = run(exe, "segments", 2, *labels).split(" | ")
    assert ints(off) == [0, 1100, 1172]
    chunks, fold_off = gram.split("/")
    assert chunks == "0+512,512+512,1024+76,1100+72" and fold_off == "0,3,4"
    chunks, fold_off = rss.split("/")
    assert chunks.split(",")[:2] == ["0+64", "64+64"] and chunks.split(",")[-1] == "1164+6"
    assert ints(fold_off) == [0, 18, 20]


def test_segment_sweep(exe):
    last = run(exe, "sweep").splitlines()[-1].split()
    assert last[0] == "sweep" and int(last[1]) >= 400 and int(last[2]) == 0


def batches(exe, F, C, k=3, T=100, burn=0, thin=1, budget=1 << 60):
    head, tail = run(exe, "batches", F, C, k, T, burn, thin, budget).split("|")
    kept, per_chain = (int(v) for v in head.split())
    out = []
    for item in tail.split():
        if item == "none":
            return kept, per_chain, None
        folds, launches = item.split(":")
        f0, f1 = (int(v) for v in folds.split("-"))
        out.append((f0, f1, [tuple(int(v) for v in l.split("+")) for l in launches.split(",")]))
    return kept, per_chain, out


def test_launch_split_at_the_grid_bound(exe):
    # F x C = 2048: one launch; 2049 = 3 x 683 and 2100 = 30 x 70: a second launch with the rest
    assert batches(exe, 2, 1024)[2] == [(0, 2, [(0, 2048)])]
    assert batches(exe, 3, 683)[2] == [(0, 3, [(0, 2048), (2048, 1)])]
    assert batches(exe, 30, 70)[2] == [(0, 30, [(0, 2048), (2048, 52)])]
    assert batches(exe, 1024, 5)[2] == [(0, 1024, [(0, 2048), (2048, 2048), (4096, 1024)])]


def test_batches_follow_the_memory_budget(exe):
    kept, per_chain, b = batches(exe, 7, 2, k=3, T=100, burn=10, thin=4)
    assert kept == 23                                            # ceil(90 / 4)
    assert per_chain == (100 * 3 + 100 + 100 * 4 + 23 * 4) * 8   # xi, gamma, rotated and kept draws
    assert b == [(0, 7, [(0, 14)])]
    fold = 2 * per_chain
    # room for three folds at a time: batches of 3, 3 and 1 folds, chains numbered globally
    assert batches(exe, 7, 2, T=100, burn=10, thin=4, budget=3 * fold + 5)[2] == \
        [(0, 3, [(0, 6)]), (3, 6, [(6, 6)]), (6, 7, [(12, 2)])]
    assert batches(exe, 7, 2, T=100, burn=10, thin=4, budget=fold)[2] == \
        [(f, f + 1, [(2 * f, 2)]) for f in range(7)]
    assert batches(exe, 7, 2, T=100, burn=10, thin=4, budget=fold - 1)[2] is None   # not one fold fits


def test_refusals(exe):
    ok = [0, 1, 0, 1, 0, 1]
    assert run(exe, "check", 2, 2, *ok) == "ok"
    assert "fold 1 is empty" in run(exe, "check", 1, 3, 0, 2, 0, 2, 0, 2)
    assert re.search(r"fold 0: its training set has 1 rows, fewer than k = 2",
                     run(exe, "check", 2, 2, 0, 0, 0, 1))
    assert "k must be between 1 and 64" in run(exe, "check", 65, 2, *([0, 1] * 40))
    assert "k must be between" not in run(exe, "check", 64, 2, *([0, 1] * 70))
    assert "n_folds must be between 2 and 1024" in run(exe, "check", 1, 1, 0, 0, 0)
    assert "n_folds must be between 2 and 1024" in run(exe, "check", 1, 1025, *range(1025))
    assert run(exe, "check", 1, 1024, *range(1024)) == "ok"
    assert "outside 0 .. 1" in run(exe, "check", 1, 2, 0, 1, 2)
    assert "outside 0 .. 1" in run(exe, "check", 1, 2, 0, 1, -1)


def test_header_declares_and_python_binds_the_entry_point():
    with open(HEADER) as f:
        text = f.read()
    m = re.search(r"int bmc_kfold_cv\(([^;]*)\);", text)
    assert m, "include/pybmc_amd.h does not declare bmc_kfold_cv"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 21
    assert "fold" in params[7] and "n_folds" in params[8] and "seeds" in params[17]
    assert "draws_out" in params[20]
    restype, argtypes = _lib.PROTOTYPES["bmc_kfold_cv"]
    assert len(argtypes) == len(params)
    assert hasattr(_lib.Context, "kfold_cv")
    assert issubclass(_lib.SingularFoldError, _lib.BmcError)
