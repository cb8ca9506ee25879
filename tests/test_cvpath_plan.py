"""CPU checks of the component-path plan (bmc_cvpath_plan.h; g++ builds tests/cvpath_plan_check.cpp):
the candidate list, the split of the m x F problems into batches and of a batch's chains into
launches of one width class, the descriptors, the memory estimate, and the declaration and binding
of bmc_cv_path.  The driver is built a second time with the address and undefined-behaviour
sanitizers and run on its own."""
import os
import re
import shutil
import subprocess

import pytest

from pybmc_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "pybmc_amd.h")


def build(tmp, name, *flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is required")
    out = tmp / name
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *flags,
                        os.path.join(HERE, "cvpath_plan_check.cpp"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(out)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("cvpath_plan"), "cvpath_plan_check")


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip()


def plan(exe, F, C, comps, T=100, burn=0, thin=1, budget=1 << 60):
    kept, per, tail = run(exe, "plan", F, C, T, burn, thin, budget, *comps).split("|")
    per = [int(v) for v in per.split()]
    items = tail.split()
    if items and items[0] == "none":
        return int(kept), per, ("none", int(items[1]), int(items[2]))
    out = []
    for item in items:
        head, launches = item.split(":")
        span, nbytes = head.split("/")
        p0, p1 = (int(v) for v in span.split("-"))
        ls = []
        for l in launches.split(","):
            kmax, rest = l.split("@")
            c0, nc = rest.split("+")
            ls.append((int(kmax), int(c0), int(nc)))
        out.append((p0, p1, int(nbytes), ls))
    return int(kept), per, out


def chain_bytes(k, T, kept):
    return (T * k + T + T * (k + 1) + kept * (k + 1)) * 8   # cv_chain_bytes: xi, gamma, rotated, kept


def per89(exe):
    """room for two k = 8 problems and one of k = 9 (T = 10, C = 1), not for a second of k = 9"""
    return 2 * chain_bytes(8, 10, 10) + chain_bytes(9, 10, 10)


def test_candidate_lists(exe):
    assert run(exe, "check", 3, 1, 2, 3) == "ok"
    assert run(exe, "check", 64, 1, 8, 9, 64) == "ok"
    assert "strictly increasing" in run(exe, "check", 5, 2, 1)
    assert "strictly increasing" in run(exe, "check", 5, 2, 2)
    assert "outside 1 .. 5" in run(exe, "check", 5, 0, 1)
    assert "outside 1 .. 5" in run(exe, "check", 5, 1, 6)
    assert "at least one candidate" in run(exe, "check", 5)
    assert "k must be between 1 and 64" in run(exe, "check", 65, 1)


def test_one_launch_per_width_class_widest_first(exe):
    # F = 2, C = 3: problems 0 .. 15, candidate j owns problems 2 j, 2 j + 1, chains 6 j .. 6 j + 5
    comps = (1, 8, 9, 16, 17, 32, 33, 64)
    kept, per, b = plan(exe, 2, 3, comps, T=100, burn=10, thin=4)
    assert kept == 23
    assert per == [3 * chain_bytes(k, 100, 23) for k in comps]       # bytes per problem
    assert b == [(0, 16, 2 * sum(per), [(64, 36, 12), (32, 24, 12), (16, 12, 12), (8, 0, 12)])]


def test_launch_split_inside_a_candidate(exe):
    # 2 candidates x 30 folds x 40 chains = 2400 chains of one class: 2048 + 352
    assert plan(exe, 30, 40, (1, 2), T=20)[2][0][3] == [(8, 0, 2048), (8, 2048, 352)]
    # two classes: every class is cut on its own
    ls = plan(exe, 30, 40, (8, 9), T=20)[2][0][3]
    assert ls == [(16, 1200, 1200), (8, 0, 1200)]
    ls = plan(exe, 60, 40, (8, 9), T=20)[2][0][3]
    assert ls == [(16, 2400, 2048), (16, 4448, 352), (8, 0, 2048), (8, 2048, 352)]


def test_batches_follow_the_memory_budget(exe):
    comps = (1, 2, 3)
    kept, per, b = plan(exe, 5, 2, comps, T=300)
    assert b == [(0, 15, 5 * sum(per), [(8, 0, 30)])]
    # just over two of the largest problems: the narrow ones go three or two at a time
    kept, per, b = plan(exe, 5, 2, comps, T=300, budget=2 * per[2] + 100)
    # greedy over the problems in order: 4 x k=1 | k=1 + 2 x k=2 | 2 x k=2 | k=2 + k=3 | 2 x k=3 | 2 x k=3
    assert [x[:2] for x in b] == [(0, 4), (4, 7), (7, 9), (9, 11), (11, 13), (13, 15)]
    assert all(x[2] <= 2 * per[2] + 100 for x in b)
    assert b[1][3] == [(8, 0, 6)]                 # chains are numbered within their batch
    assert b[0][2] == 4 * per[0] and b[1][2] == per[0] + 2 * per[1] and b[3][2] == per[1] + per[2]
    # a batch that holds the end of one class and the start of the next
    b = plan(exe, 2, 1, (8, 9), T=10, budget=per89(exe))[2]
    assert [x[:2] for x in b] == [(0, 3), (3, 4)]
    assert b[0][3] == [(16, 2, 1), (8, 0, 2)] and b[1][3] == [(16, 0, 1)]
    # a budget below one problem's need is reported, not planned
    kept, per, b = plan(exe, 5, 2, comps, T=300, budget=per[2] - 1)
    assert b == ("none", 10, per[2])
    assert plan(exe, 5, 2, comps, T=300, budget=per[2])[2][-1][:2] == (14, 15)


def test_every_chain_once_under_all_invariants(exe):
    assert run(exe, "verify", 2, 1, 300, 0, 1, 1 << 60, 1, 8, 9, 16, 17, 32, 33, 64) == "ok 1"
    assert run(exe, "verify", 30, 40, 20, 0, 1, 1 << 60, 1, 2) == "ok 1"
    assert run(exe, "verify", 5, 2, 300, 37, 4, 100000, 1, 2, 3).startswith("ok ")
    assert run(exe, "verify", 5, 2, 300, 0, 1, 100, 1, 2, 3).startswith("refused 0 ")
    last = run(exe, "sweep").split()
    assert last[0] == "sweep" and int(last[1]) == 600 and int(last[2]) == 0 and int(last[3]) > 0


def test_the_driver_is_clean_under_the_sanitizers(tmp_path):
    exe = build(tmp_path, "cvpath_plan_check_san", "-g", "-fsanitize=address,undefined",
                "-fno-sanitize-recover=undefined")
    assert run(exe, "sweep").startswith("sweep 600 0")
    assert run(exe, "verify", 30, 40, 20, 0, 1, 1 << 60, 1, 2) == "ok 1"
    assert run(exe, "verify", 5, 2, 300, 37, 4, 100000, 1, 2, 3).startswith("ok ")


def test_header_declares_and_python_binds_the_entry_point():
    with open(HEADER) as f:
        text = f.read()
    m = re.search(r"int bmc_cv_path\(([^;]*)\);", text)
    assert m, "include/pybmc_amd.h does not declare bmc_cv_path"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    k = re.search(r"int bmc_kfold_cv\(([^;]*)\);", text).group(1).replace("\n", " ").split(",")
    assert len(params) == len(k) + 2 == 23
    assert [p.split()[-1] for p in params[:18]] == [p.split()[-1] for p in k[:18]]
    assert "const int32_t* comps" in params[18] and "int32_t n_comps" in params[19]
    assert "draws_out" in params[22]
    restype, argtypes = _lib.PROTOTYPES["bmc_cv_path"]
    assert len(argtypes) == len(params)
    assert hasattr(_lib.Context, "cv_path")
    assert _lib.ABI_VERSION == 4 and "#define PYBMC_AMD_ABI_VERSION 4" in text
