"""CPU checks of the Student-t sampler's host plan (bmc_robust_plan.h; g++ builds
tests/robust_plan_check.cpp): the row slabs of the four waves, the launch lists, the buffer sizes and
the refusals."""
import math
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

NS = (1, 3, 63, 64, 65, 255, 256, 257, 629, 1237, 10000)
KS = (1, 3, 15, 16, 17, 32)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is required")
    out = tmp_path_factory.mktemp("robust_plan") / "robust_plan_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                        os.path.join(HERE, "robust_plan_check.cpp"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(out)


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip()


def max_chains_per_launch(exe):
    """What the GPU tests ask the plan for: the largest chain count of one launch."""
    return int(run(exe, "launches", 1).split("|")[0])


@pytest.mark.parametrize("n", NS)
def test_slabs_cover_every_row_once(exe, n):
    for k in KS:
        head, slabs = run(exe, "slabs", n, k).split("|")
        rpw, n_pad, tiles, pairs, kc, ldz = (int(v) for v in head.split())
        assert rpw % 4 == 0 and rpw == 4 * math.ceil(math.ceil(n / 4) / 4)   # whole k-steps, N alone
        assert n_pad == 4 * rpw and n <= n_pad < n + 16
        assert tiles == (1 if k <= 16 else 2) and ldz == 16 * tiles and ldz >= k
        assert pairs == tiles * (tiles + 1) // 2
        assert kc >= k and kc in (4, 8, 16, 32) and (kc == 4 or kc // 2 < k)
        rows = []
        for w, s in enumerate(slabs.split()):
            r0, r1 = (int(v) for v in s.split("-"))
            assert r0 == min(n, w * rpw) and r0 <= r1 <= n and r1 - r0 <= rpw   # fixed, contiguous
            rows += range(r0, r1)
        assert rows == list(range(n))


@pytest.mark.parametrize("c", (1, 3, 256, 257, 1000, 1024, 1025, 2049))
def test_launch_lists_cover_every_chain_once(exe, c):
    head, tail = run(exe, "launches", c).split("|")
    cap = int(head)
    launches = [tuple(int(v) for v in item.split("+")) for item in tail.split()]
    assert len(launches) == math.ceil(c / cap)
    chains = []
    for c0, m in launches:
        assert 1 <= m <= cap
        chains += range(c0, c0 + m)
    assert chains == list(range(c))
    assert all(m == cap for _, m in launches[:-1])


def test_buffer_sizes_are_exact(exe):
    for n, k, c, sweeps in ((1, 1, 1, 1), (629, 3, 64, 300), (1237, 17, 3, 50), (10000, 32, 256, 7)):
        ws, packed, gl = (int(v) for v in run(exe, "bytes", n, k, c, sweeps).split())
        n_pad = 16 * math.ceil(n / 16)
        assert ws == c * n * 2 * 8                              # [C][N][2] f64
        assert packed == n_pad * ((16 if k <= 16 else 32) + 1) * 8   # Z and y, padded rows
        assert gl == c * sweeps * n * 8


def test_refusals(exe):
    assert run(exe, "check", 629, 3, 0, 4.0, 2, 100, 10) == "ok"
    assert run(exe, "check", 1, 1, 0, 0.5, 1, 0, 0) == "ok"
    assert run(exe, "check", 300, 32, 0, 4.0, 1, 10, 0) == "ok"
    assert "1 <= k <= 32" in run(exe, "check", 300, 33, 0, 4.0, 1, 10, 0)
    assert "1 <= k <= 32" in run(exe, "check", 300, 0, 0, 4.0, 1, 10, 0)
    assert "nu must be positive" in run(exe, "check", 300, 3, 0, 0.0, 1, 10, 0)
    assert "nu must be positive" in run(exe, "check", 300, 3, 0, -1.0, 1, 10, 0)
    assert "nu must be positive" in run(exe, "check", 300, 3, 0, "nan", 1, 10, 0)
    assert "N >= 1" in run(exe, "check", 0, 3, 0, 4.0, 1, 10, 0)
    assert "2^32" in run(exe, "check", 2 ** 32, 3, 0, 4.0, 1, 10, 0)
    assert "float64" in run(exe, "check", 300, 3, 1, 4.0, 1, 10, 0)
    assert "n_chains" in run(exe, "check", 300, 3, 0, 4.0, 0, 10, 0)
    assert "non-negative" in run(exe, "check", 300, 3, 0, 4.0, 1, 10, -1)
    assert "iters" in run(exe, "check", 300, 3, 0, 4.0, 1, -1, 0)
