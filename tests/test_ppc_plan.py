"""plan_ppc (pybmc_amd/csrc/bmc_plan.h) on the CPU: g++ builds tests/ppc_plan_check.cpp, which
includes the header the library is built from.  Pads, grid, byte counts and refusals of the
posterior predictive check's plan."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is required")
    exe = tmp_path_factory.mktemp("ppc_plan") / "ppc_plan_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                        os.path.join(HERE, "ppc_plan_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def plan(exe, n, S, k, n_cu=256):
    r = subprocess.run([exe, "plan", str(n), str(S), str(k), str(n_cu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return dict((kv.split("=")[0], int(kv.split("=")[1])) for kv in r.stdout.split())


def test_smallest_accepted_shape(plan_exe):
    p = plan(plan_exe, 3, 2, 1)
    assert p["ok"] == 1
    assert (p["point_tiles"], p["draw_tiles"], p["n_pad"], p["S_pad"], p["k_pad"]) == (1, 1, 64, 64, 16)
    assert p["grid"] == 1 and p["rounds"] == 1
    assert p["bytes_Ap"] == 64 * 16 * 8 and p["bytes_Tp"] == 64 * 16 * 8
    # sg: sigma_s, 1 / sigma_s and the draw's centre, then the k_pad column means and the mean offset
    assert p["bytes_yo"] == 2 * 64 * 8 and p["bytes_sg"] == (3 * 64 + 16 + 16) * 8
    assert p["bytes_out"] == 2 * 10 * 8
    assert p["bytes_total"] == sum(p["bytes_" + key] for key in ("Ap", "yo", "Tp", "sg", "out"))


@pytest.mark.parametrize("n,S,k,want", [
    (33, 70, 1, (1, 2, 64, 128, 16)),
    (65, 130, 3, (2, 3, 128, 192, 16)),
    (150, 64, 17, (3, 1, 192, 64, 32)),
    (200, 257, 33, (4, 5, 256, 320, 48)),
    (629, 300, 3, (10, 5, 640, 320, 16)),
    (10000, 50000, 32, (157, 782, 10048, 50048, 32)),
])
def test_named_shapes(plan_exe, n, S, k, want):
    p = plan(plan_exe, n, S, k)
    assert (p["point_tiles"], p["draw_tiles"], p["n_pad"], p["S_pad"], p["k_pad"]) == want
    assert p["grid"] == p["draw_tiles"]          # one workgroup per 64 draws: no split over points
    assert p["bytes_out"] == S * 10 * 8


def test_the_grid_does_not_depend_on_the_device(plan_exe):
    """Only `rounds`, which nothing on the device reads, follows the CU count."""
    a, b = plan(plan_exe, 10000, 50000, 32, 256), plan(plan_exe, 10000, 50000, 32, 8)
    assert {k: v for k, v in a.items() if k != "rounds"} == {k: v for k, v in b.items() if k != "rounds"}
    assert a["rounds"] == 2 and b["rounds"] == 49        # 782 workgroups over 512 and 16 slots
    assert plan(plan_exe, 629, 16384, 3, 256)["rounds"] == 1    # 256 workgroups: half the slots idle


@pytest.mark.parametrize("n,S,k", [(2, 100, 3), (0, 100, 3), (3, 1, 3), (100, 100, 0), (100, 100, 257),
                                   (2 ** 31 + 1, 100, 3)])
def test_refusals(plan_exe, n, S, k):
    p = plan(plan_exe, n, S, k)
    assert p["ok"] == 0 and p["bytes_total"] == 0


def test_limits_are_accepted(plan_exe):
    assert plan(plan_exe, 2 ** 31, 2, 256)["ok"] == 1
    assert plan(plan_exe, 3, 2, 256)["k_pad"] == 256


def test_sweep(plan_exe):
    r = subprocess.run([plan_exe, "sweep"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    plans, fails = r.stdout.split()[-2:]
    assert int(plans) == 13 * 12 * 10 * 6 and int(fails) == 0
