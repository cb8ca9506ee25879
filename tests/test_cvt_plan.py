"""CPU checks of the Student-t cross-validation plan (bmc_cvt_plan.h; g++ builds
tests/cvt_plan_check.cpp): the descriptor of every fold's packed training rows, the batches of whole
folds under a byte budget, the launch split at 1024 workgroups, the refusals, and the declaration
and binding of bmc_kfold_cv_t / bmc_kfold_cv_tv."""
import os
import re
import shutil
import subprocess

import pytest

from pybmc_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "pybmc_amd.h")

# fold sizes 1 / 5 / 17 of n = 23
LABELS = [0] + [1] * 5 + [2] * 17


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is required")
    out = tmp_path_factory.mktemp("cvt_plan") / "cvt_plan_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                        os.path.join(HERE, "cvt_plan_check.cpp"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(out)


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip()


def plan(exe, labels, k=2, C=2, T=40, burn=0, thin=1, G=0, budget=1 << 60):
    """(kept, bytes per fold, batches or None); a batch is (f0, f1, z_len, yv_len, rows, folds,
    launches), a fold (fold, n_train, rows_per_wave, rows_padded, z_off, yv_off, row0)."""
    lines = run(exe, "plan", k, C, T, burn, thin, G, budget, *labels).splitlines()
    head = [int(v) for v in lines[0].split()]
    if lines[1].startswith("none"):
        return head[0], head[1:], None, tuple(int(v) for v in lines[1].split()[1:])
    out = []
    for line in lines[1:]:
        top, folds, launches = line.split(" : ")
        span, z_len, yv_len, rows = top.split()
        f0, f1 = (int(v) for v in span.split("-"))
        out.append((f0, f1, int(z_len), int(yv_len), int(rows),
                    [tuple(int(v) for v in f.split(",")) for f in folds.split(" ; ")],
                    [tuple(int(v) for v in l.split("+")) for l in launches.split(",")]))
    return head[0], head[1:], out, None


def test_descriptors_of_unequal_folds(exe):
    kept, per_fold, batches, _ = plan(exe, LABELS)
    assert kept == 40 and len(batches) == 1
    f0, f1, z_len, yv_len, rows, folds, launches = batches[0]
    assert (f0, f1) == (0, 3) and launches == [(0, 6)]
    # n_train 22 / 18 / 6: 6, 5 and 2 k-steps of 4 rows over 4 waves -> 8 / 8 / 4 rows per wave.  At
    # n_train = 6 the waves' slabs are [0, 4), [4, 6), [6, 6), [6, 6): two of them are empty.
    assert [f[1] for f in folds] == [22, 18, 6]
    assert [f[2] for f in folds] == [8, 8, 4]
    assert [f[3] for f in folds] == [32, 32, 16]
    assert [max(0, min(6, (w + 1) * 4) - min(6, w * 4)) for w in range(4)] == [4, 2, 0, 0]
    # the packed rows [rows_padded][16] one fold after the other, then the targets; two chains a
    # fold own n_train rows of ws / wsum each
    assert [f[4] for f in folds] == [0, 32 * 16, 64 * 16] and z_len == 80 * 16
    assert [f[5] for f in folds] == [0, 32, 64] and yv_len == 80
    assert [f[6] for f in folds] == [0, 44, 80] and rows == 2 * (22 + 18 + 6)
    # bytes: the replicated rows, and per chain xi, gamma, ws, wsum, the draws after burn, the kept
    for nt, padded, got in zip((22, 18, 6), (32, 32, 16), per_fold):
        assert got == padded * 17 * 8 + 2 * (40 * 2 + 40 + 3 * nt + 40 * 3 + 40 * 3) * 8


def test_two_column_tiles_and_the_nu_grid_count(exe):
    labels = [i % 3 for i in range(150)]
    kept, per_fold, batches, _ = plan(exe, labels, k=17, C=1, T=10, burn=4, thin=3, G=7)
    assert kept == 2
    folds = batches[0][5]
    assert [f[1] for f in folds] == [100, 100, 100] and [f[2] for f in folds] == [28, 28, 28]
    assert [f[4] for f in folds] == [0, 112 * 32, 224 * 32]          # ldz = 32
    chain = (10 * 17 + 10 + 3 * 100 + 6 * 18 + 2 * 18) * 8 + (6 + 2) * 4
    assert per_fold[0] == 112 * 33 * 8 + 4 * 7 * 8 + chain


def test_batches_of_whole_folds_under_a_budget(exe):
    kept, per_fold, batches, _ = plan(exe, LABELS)
    a, b, c = per_fold
    # room for the first two folds together but not the third with them
    _, _, two, _ = plan(exe, LABELS, budget=a + b + c - 1)
    assert [(x[0], x[1]) for x in two] == [(0, 2), (2, 3)]
    assert [f[4] for f in two[1][5]] == [0] and [f[6] for f in two[1][5]] == [0]   # offsets restart
    assert two[0][6] == [(0, 4)] and two[1][6] == [(0, 2)]                          # chains local to the batch
    _, _, one, _ = plan(exe, LABELS, budget=max(per_fold))
    assert [(x[0], x[1]) for x in one] == [(0, 1), (1, 2), (2, 3)]
    # not one fold fits: the largest fold is named with its need
    _, _, none, why = plan(exe, LABELS, budget=max(per_fold) - 1)
    assert none is None and why == (0, a)


def test_launch_split_at_1024_chains(exe):
    labels = [i % 30 for i in range(60)]
    _, _, batches, _ = plan(exe, labels, C=35, T=20)
    assert batches[0][6] == [(0, 1024), (1024, 26)]
    _, _, batches, _ = plan(exe, [0, 1] * 4, C=512, T=5)
    assert batches[0][6] == [(0, 1024)]
    _, _, batches, _ = plan(exe, [0, 1, 2] * 4, C=683, T=5)
    assert batches[0][6] == [(0, 1024), (1024, 1024), (2048, 1)]


def check(exe, labels, k=2, C=2, T=40, burn=0, thin=1, nu=4.0, G=0):
    return run(exe, "check", k, C, T, burn, thin, nu, G, *labels)


def test_refusals(exe):
    ok = [0, 1] * 40
    assert check(exe, ok) == "ok" and check(exe, ok, G=7) == "ok" and check(exe, ok, k=32) == "ok"
    assert "supports 1 <= k <= 32 columns; got 33" in check(exe, ok, k=33)
    assert "fold 1 is empty" in check(exe, [0, 2, 0, 2, 0, 2])
    assert re.search(r"fold 0: its training set has 1 rows, fewer than k = 2", check(exe, [0, 0, 0, 1]))
    assert "n_folds must be between 2 and 1024" in check(exe, [0, 0, 0])
    assert "n_chains must be between 1 and 65535" in check(exe, ok, C=0)
    assert "iters must be between" in check(exe, ok, T=0)
    assert "need 0 <= burn < iters and thin >= 1" in check(exe, ok, burn=40)
    assert "need 0 <= burn < iters and thin >= 1" in check(exe, ok, thin=0)
    assert "at least 2 draws per fold" in check(exe, ok, C=1, T=3, burn=2)
    assert "nu must be positive and finite" in check(exe, ok, nu=0.0)
    assert "nu must be positive and finite" in check(exe, ok, nu=-1.0)
    assert "the nu grid needs 1 <= n_grid <= 64 values; got 65" in check(exe, ok, G=65)


def test_header_declares_and_python_binds_both_entry_points():
    with open(HEADER) as f:
        text = f.read()
    assert "#define PYBMC_AMD_ABI_VERSION 4" in text
    for name, count, last in (("bmc_kfold_cv_t", 23, "weight_out"), ("bmc_kfold_cv_tv", 27, "nu_idx_out")):
        m = re.search(r"int %s\(([^;]*)\);" % name, text)
        assert m, f"include/pybmc_amd.h does not declare {name}"
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        assert len(params) == count and last in params[-1]
        assert "fold" in params[7] and "n_folds" in params[8] and "seeds" in params[17]
        restype, argtypes = _lib.PROTOTYPES[name]
        assert len(argtypes) == len(params)
    assert hasattr(_lib.Context, "kfold_cv_t")
