"""The launch plans of the chain-diagnostics kernels on the CPU: g++ builds tests/diag_plan_check.cpp
from the header the kernels are launched from (bmc_diag_plan.h: moment_plan, acov_plan).  Every
figure of every shape of tests/diag_cases.py is pinned, and a sweep over C in 1..300, n in 4..3000,
n_active in 1..4200 and the lag blocks of the ESS scan asserts what the kernels rely on: rps a
multiple of the 128-row tile, the row splits tiling [0, n) once, (MG - 1) spg < 2C <= MG spg, one
16 x 64 f64 slab of scratch per workgroup; for the moments, splits covering [0, n) once and no
more of them than started blocks of 256 rows (S = 1 or 256 (S - 1) < n: the splits are even, so
n = 257 gives 129 + 128 rows, never a short tail).

The class each shape of the end-to-end GPU tests reaches, first lag block [0, 64) (the later blocks
[64, 192), [192, 448) change nlc alone); tiles = ceil(n / 128):

  test, (C, T, burn, P)                          ncc  MG  spg  S   rps  tiles  moments S
  diagnostics iid / ar1_0.5 (4, 3000, 0, 5|3)      1   8    1  12  128    12     6
  diagnostics ar1_0.99 (4, 6000, 0, 3)             1   8    1  24  128    24    12
  diagnostics ar1_0.999 (2, 20000, 0, 2)           1   4    1  79  128    79    40
  diagnostics shifted (4, 1000, 0, 3)              1   8    1   4  128     4     2
  diagnostics large_mean (4, 2000, 0, 2)           1   8    1   8  128     8     4
  diagnostics odd (3, 1001, 100|0, 4)              1   6    1   4  128     4     2
  diagnostics counts (1, 500, 10, 1)               1   2    1   2  128     2     1
  diagnostics counts (64, 200, 10, 33)             3 128    1   1  128     1     1
  diagnostics counts (2, 300, 10, 257)            17   4    1   2  128     2     1
  diagnostics subset (3, 800, 0, 5)                1   6    1   4  128     4     2
  diagnostics degenerate (2, 300, 0, 4)            1   4    1   2  128     2     1
  diagnostics bitwise (8, 4000, 3, 17)             2  16    1  16  128    16     8
  diagnostics run_chains (8, 4000, 0, 6)           1  16    1  16  128    16     8
  rank, 4 derived columns per call: (4, 2000)      1   8    1   8  128     8     4
        (3, 700) 6/3/3, (4, 3000) 8/12/12, (2, 400|300|500) 4/2/2, (1, 4096) 2/16/16,
        (4, 8202) 8/33/33, (1, 8) 2/1/1: MG / S / tiles, always ncc = 1, spg = 1, rps = 128

Everywhere spg = 1 and MG spg = 2C: no group of several half-chains, no clipped last group, never
the units >= 2048 branch; and in the first three blocks S = tiles, one tile per split.  Two inputs
scan further (the FFT reference puts their max_lag at 9997 and 703): ar1_0.999 runs the blocks
[448, 960) .. [8128, 9944) with S = 40, 27, 16, 8, 16 and rps = 256 .. 1280, and the bitwise test
[448, 960) with S = 8, rps = 256.  There a split does hold several tiles, but all that is seen of
them is the ESS (rtol 1e-9) of two columns, or a second run of the same code.  The shapes added to
test_chain_and_column_counts, (256, 40, 10, 300): ncc 19, MG 103, spg 5 and (32, 1400, 10, 100):
S 3, rps 256 in the first block, and tests/diag_cases.py close this."""
import os
import shutil
import subprocess

import pytest

import diag_cases as dc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is required")
    out = tmp_path_factory.mktemp("diag_plan") / "diag_plan_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                        os.path.join(HERE, "diag_plan_check.cpp"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(out)


def plan(exe, C, T, burn, P, n_active, n_lags):
    r = subprocess.run([exe, "plan", *map(str, (C, T, burn, P, n_active, n_lags))],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    acov, moments = (line.split() for line in r.stdout.splitlines())
    assert acov[0] == "acov" and moments[0] == "moments"
    return tuple(map(int, acov[1:])), tuple(map(int, moments[1:]))


@pytest.mark.parametrize("tag", list(dc.ACOV_CASES))
def test_acov_plan_of_every_table_shape(exe, tag):
    c = dc.ACOV_CASES[tag]
    C, T, burn, P = c["shape"]
    n = (T - burn) // 2
    acov, _ = plan(exe, C, T, burn, P, c.get("n_active", P), c["lags"][1])
    ncc, nlc, MG, spg, S, rps = c["plan"]
    assert acov[:6] == c["plan"]
    assert acov[6] == MG * ncc * nlc * S and acov[7] == acov[6] * 16 * 64 * 8
    # the class the row is in the table for
    tiles = -(-n // 128)
    per_split = rps // 128
    want = {"A1": n == 4, "A2": n < 64 and (T - burn) % 2 == 1,
            "B": tiles == 2 and S == 2 and n % 128 != 0,
            "C": n == 150 and c["lags"][0] > 0 and sum(c["lags"]) > n and P % 16 == 4,
            "D": per_split == 2 and tiles == 9 and n - (S - 1) * rps == 76,
            "D0": per_split == 2 and n - (S - 1) * rps == 76 and c["lags"][0] == 0 and nlc == 4,
            "E": spg == 3 and MG * spg - 2 * C == 1,
            "F": spg == 2 and S == 1 and tiles == 3,
            "F0": spg == 2 and S == 1 and tiles == 3 and c["lags"][0] == 0,
            "G": ncc * nlc >= 2048 and MG == 1 and spg == 2 * C and tiles == 2 and c["lags"][1] > n,
            "H": c.get("n_active", P) < P and S == tiles == 3}[tag]
    assert want, (tag, acov)


@pytest.mark.parametrize("key", list(dc.MOMENT_CASES), ids=dc.moment_id)
def test_moment_plan_of_every_table_shape(exe, key):
    C, T, burn, P = key
    _, (n_seq, ncc, S, rps, nbytes) = plan(exe, C, T, burn, P, P, 1)
    assert n_seq == (3 if (T - burn) % 2 else 2) * C
    assert (ncc, S, rps) == dc.MOMENT_CASES[key]
    assert nbytes == n_seq * S * 2 * P * 8


def test_moment_plans_of_the_acov_shapes(exe):
    """The moments classes the acov rows add: five row splits (D), two with six column chunks
    (F: 3 chunks, E: 6), 64 chunks (G)."""
    got = {}
    for tag, c in dc.ACOV_CASES.items():
        C, T, burn, P = c["shape"]
        got[tag] = plan(exe, C, T, burn, P, c.get("n_active", P), c["lags"][1])[1][1:4]
    assert got == {"A1": (1, 1, 4), "A2": (1, 1, 9), "B": (1, 1, 130), "C": (1, 1, 150),
                   "D": (1, 5, 220), "D0": (1, 5, 220), "E": (6, 1, 40),
                   "F": (3, 2, 150), "F0": (3, 2, 150), "G": (64, 1, 130),
                   "H": (1, 2, 150)}


def test_the_added_end_to_end_shapes(exe):
    # test_chain_and_column_counts runs them with burn = 10; first lag block
    acov, _ = plan(exe, 256, 40, 10, 300, 300, 15)
    assert acov[:6] == (19, 1, 103, 5, 1, 128) and 103 * 5 - 512 == 3      # last group clipped by 3
    acov, _ = plan(exe, 32, 1400, 10, 100, 100, 64)
    assert acov[:6] == (7, 1, 64, 1, 3, 256) and -(-695 // 128) == 6       # two tiles per split


def test_sweep(exe):
    r = subprocess.run([exe, "sweep"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    word, plans, failures = r.stdout.split()
    assert word == "sweep" and int(plans) > 10_000_000 and int(failures) == 0
