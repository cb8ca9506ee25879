"""CPU checks of the nu-grid part of the Student-t sampler's host plan (bmc_robust_plan.h; g++ builds
tests/robust_nu_plan_check.cpp): the refusals, the table the kernel keeps in LDS, and the constants
c_g = n (h log h - lgamma h) + log w against a long-double evaluation."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is required")
    out = tmp_path_factory.mktemp("robust_nu_plan") / "robust_nu_plan_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                        os.path.join(HERE, "robust_nu_plan_check.cpp"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(out)


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip()


def test_refusals(exe):
    assert run(exe, "max") == "64"
    assert run(exe, "check", 0, "4") == "ok"
    assert run(exe, "check", 1, "1.5:0", "4:2", "50:0.5") == "ok"
    assert run(exe, "check", 63, *[f"{1 + g}" for g in range(64)]) == "ok"
    assert "1 <= n_grid <= 64" in run(exe, "check", 0, *[f"{1 + g}" for g in range(65)])
    assert "1 <= n_grid <= 64" in run(exe, "check", 0)
    assert "strictly increasing" in run(exe, "check", 0, "2", "2")
    assert "strictly increasing" in run(exe, "check", 0, "2", "1")
    for bad in ("0", "-1", "inf", "nan"):
        assert "positive and finite" in run(exe, "check", 0, "1", bad)
    for bad in ("-1", "inf", "nan"):
        assert "non-negative and finite" in run(exe, "check", 0, f"1:{bad}", "2:1")
    assert "at least one" in run(exe, "check", 0, "1:0", "2:0")
    assert "must index" in run(exe, "check", 2, "1", "2")
    assert "must index" in run(exe, "check", -1, "1", "2")
    assert "positive prior weight" in run(exe, "check", 0, "1:0", "2:1")


def test_table_rows(exe):
    grid, weight, n = (1.5, 4.0, 50.0), (0.25, 0.0, 3.0), 629
    rows = [[float(v) for v in line.split()]
            for line in run(exe, "table", n, *[f"{g!r}:{w!r}" for g, w in zip(grid, weight)]).splitlines()]
    assert len(rows) == 3
    for (nu, shape, h, c), g, w in zip(rows, grid, weight):
        assert nu == g and shape == (g + 1.0) / 2.0 and h == g / 2.0
        if w == 0.0:
            assert c == -math.inf
        else:
            want = n * (h * math.log(h) - math.lgamma(h)) + math.log(w)
            assert abs(c - want) <= 4 * 2.0 ** -52 * n * abs(want)


@pytest.mark.parametrize("n", (3, 629, 200_000))
def test_consts_against_long_double(exe, n):
    """Relative bound 4 * 2^-52 * n: the rounding of the few operations of c_g."""
    worst = 0.0
    for nu in np.concatenate([np.geomspace(0.5, 200.0, 40), [0.5, 1.0, 2.0, 4.0, 200.0]]):
        c, rel = (float(v) for v in run(exe, "consts", n, repr(float(nu))).split())
        assert np.isfinite(c)
        worst = max(worst, rel)
        assert rel <= 4 * 2.0 ** -52 * n, (n, nu, rel)
    print(f"n = {n}: largest relative deviation {worst:.3e} (bound {4 * 2.0 ** -52 * n:.3e})")
