"""The sigma column of a chain's last rows (-m gpu).  In the role-specific loop copies the leader
hands its (sp, g) pair to the recording wave in the idle slot of the exchange, one barrier later
than it used to, so the recorder stores the sigma of row t - 2 during iteration t and the last TWO
rows' sigma are written behind the loop -- the last one from words of its own.  A leader that
records itself (a group of one wave) keeps the pair in registers and owes one row.  A chain of T
iterations is a prefix of the chain of 65 on the same streams (leader_stream_cases.streams), so
the rows a short chain writes behind its loop are set against the rows the long chain writes
inside it: equal bit for bit, sigma column included."""
import functools

import numpy as np
import pytest

import leader_stream_cases as lc
from gpu_common import gpu_ctx

pytestmark = pytest.mark.gpu

# name: (n, k, tuning keywords, what the launch must report)
GEOMETRIES = {
    "g2_recorder_is_wave_1": (640, 16, dict(groups_per_chain=2), dict(groups_per_chain=2, waves_per_group=5)),
    "g32_leader_records": (640, 16, dict(groups_per_chain=32), dict(groups_per_chain=32, waves_per_group=1)),
    "headline": (10000, 32, dict(), dict(groups_per_chain=32, waves_per_group=5)),
}


def run(name, T):
    n, k, tuning, want = GEOMETRIES[name]
    ctx = gpu_ctx()
    lc.load(ctx, n, k)
    ctx.set_tuning(**tuning)
    try:
        out, st = lc.run_replay(ctx, n, k, T)     # (raises unless the launch reports BMC_OK)
    finally:
        ctx.set_tuning()
    lc.check_stats(name, st, want)
    return out[0]


@functools.lru_cache(maxsize=None)
def long_chain(name):
    """The chain of T_MAX = 65 iterations: every row but the last two has its sigma from inside the loop."""
    out = run(name, lc.T_MAX)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("T", [1, 2, 3, 4])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_short_chain_is_the_head_of_the_long_one(name, T):
    want = long_chain(name)[:T]
    out = run(name, T)
    assert out.shape == want.shape == (T, GEOMETRIES[name][1] + 1)
    assert np.all(np.isfinite(want)) and np.all(want[:, -1] > 0)
    print(f"{name} T={T}: sigma {out[:, -1]} want {want[:, -1]}")
    assert np.array_equal(out, want), (name, T, out[:, -1], want[:, -1])


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_no_iterations_give_no_rows(name):
    out = run(name, 0)
    assert out.shape == (0, GEOMETRIES[name][1] + 1)


def test_long_chain_is_the_recorded_golden():
    """The reference of this file is itself pinned: the 65-iteration chains are the goldens of
    tests/test_leader_stream_gpu.py, recorded before the hand-over moved."""
    for name, case in [("g2_recorder_is_wave_1", "k16_g2_t65"), ("g32_leader_records", "k16_g32_t65"),
                       ("headline", "headline_t65")]:
        assert np.array_equal(long_chain(name), np.load(lc.golden_path(case), allow_pickle=False)), name
