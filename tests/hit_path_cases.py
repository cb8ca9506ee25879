"""The cases of tests/test_hit_path_gpu.py and scripts/record_hit_path_golden.py: the launches
that reach what the leader's gather decides on -- the tags of ALL 64 lanes, where the lanes past
the last granule read granule 0 -- and the out-of-line floor of its sigma2 step.

  k16_g{G}_{scope}  n = 640, k = 16, T = 65, G = 2, 3, 5, 31, 32 groups (4 .. 64 granules, so that
                    up to 60 lanes read granule 0 beside their owners), in the scope the placement
                    check finds ("auto") and with agent scope forced
  headline_n4096    k = 32, G = 32 at the smallest n with two waves per group: the instantiation
                    the benchmark measures
  k16_g5_t{T}       T = 1, 2, 3: both parities of the exchange slot and the recorder's tail
  stale_a, stale_b  two launches back to back on one context, device generator, seeds of their own
  trio_g3           three chains with streams of their own in one launch; chain 0 also runs alone
  floor_g2          y in the column space of X and nu0 s20 = 1e-12: the sigma2 step's floor is hit
                    in some iterations and not in others (the Gamma stream decides, see below)

All but the stale pair run in replay mode on the seeded streams of leader_stream_cases; the chains
are compared with the bits of the commit the goldens were recorded at (the parent of the change
that took the `need` mask out of the gather and the floor's selects off the way to the draw), not
with the oracle.  One module builds the inputs for the recorder and for the test.

A golden is tests/golden/hit_path/<name>.npy: ONE chain [T, k + 1]; trio_g3 keeps its launch's
three chains, [3, T, k + 1].
"""
import functools
import os

import numpy as np

import leader_stream_cases as lc

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hit_path")
HEADLINE_KERNEL = "gibbs_loop_kernel<double, 1, 0, 32, 1, false, false, true>"
T_LONG = 65

# name: (n, k, tuning keywords, T, what the launch must report)
CASES = {}
for _G in (2, 3, 5, 31, 32):
    CASES[f"k16_g{_G}_auto"] = (640, 16, dict(groups_per_chain=_G), T_LONG, dict(groups_per_chain=_G))
    CASES[f"k16_g{_G}_agent"] = (640, 16, dict(groups_per_chain=_G, force_agent_scope=1), T_LONG,
                                 dict(groups_per_chain=_G, xcd_local_chains=0))
HEADLINE = "headline_n4096"
CASES[HEADLINE] = (4096, 32, dict(groups_per_chain=32), T_LONG, dict(groups_per_chain=32, waves_per_group=2))
for _T in (1, 2, 3):
    CASES[f"k16_g5_t{_T}"] = (640, 16, dict(groups_per_chain=5), _T, dict(groups_per_chain=5))

STALE = ("stale_a", "stale_b")
STALE_SEEDS = (21, 22)
STALE_TUNING = dict(groups_per_chain=3)
TRIO = "trio_g3"
TRIO_TUNING = dict(groups_per_chain=3)
FLOOR = "floor_g2"
FLOOR_TUNING = dict(groups_per_chain=2)
FLOOR_SHAPE = (640, 16)
SIGMA2_FLOOR = 1e-6


def golden_path(name):
    return os.path.join(GOLDEN_DIR, name + ".npy")


def run_case(ctx, name):
    """Returns (chain [T, k + 1], stats); asserts that the launch had the geometry asked for."""
    n, k, tuning, T, want = CASES[name]
    lc.load(ctx, n, k)
    ctx.set_tuning(**tuning)
    try:
        out, st = lc.run_replay(ctx, n, k, T)
    finally:
        ctx.set_tuning()
    lc.check_stats(name, st, want)
    return out[0], st


def run_stale(ctx):
    """Two launches back to back on one context, the device generator on seeds of their own.
    Returns ([chain a, chain b], [stats a, stats b])."""
    lc.load(ctx, 640, 16)
    ctx.set_tuning(**STALE_TUNING)
    try:
        runs = [ctx.gibbs_run(1, T_LONG, seeds=[s]) for s in STALE_SEEDS]
    finally:
        ctx.set_tuning()
    for _, st in runs:
        lc.check_stats("stale", st, STALE_TUNING)
    return [out[0] for out, _ in runs], [st for _, st in runs]


def run_trio(ctx):
    """Chains on streams 0, 1, 2 in one launch, and chain 0 alone.  Returns (trio [3, T, k + 1],
    alone [T, k + 1], stats)."""
    lc.load(ctx, 640, 16)
    ctx.set_tuning(**TRIO_TUNING)
    try:
        trio, st = lc.run_replay(ctx, 640, 16, T_LONG, (0, 1, 2))
        alone, st1 = lc.run_replay(ctx, 640, 16, T_LONG, (0,))
    finally:
        ctx.set_tuning()
    for s in (st, st1):
        lc.check_stats(TRIO, s, TRIO_TUNING)
    assert st["n_chains"] == 3 and st["launches"] == 1, st
    return trio, alone[0], st


@functools.lru_cache(maxsize=None)
def floor_problem():
    """(y, X, prior, xi [T, k], g [T]): y = X b exactly, so rss is the draw's own scatter, about
    k sigma2, and scale_post / g falls under 1e-6 whenever g is an ordinary Gamma((1 + n) / 2)
    variate (~320) -- the step is floored and the chain sits at sigma2 = 1e-6.  Every fourth
    variate is 0.5 instead: that step gives sigma2 ~ k 1e-6 and is not floored, nor is the one
    after it."""
    n, k = FLOOR_SHAPE
    rng = np.random.default_rng(640016)
    X = np.asfortranarray(rng.standard_normal((n, k)) / np.sqrt(n))
    y = X @ rng.standard_normal(k)
    xi, g = (a.copy() for a in lc.streams(n, k, 5))
    g[2::4] = 0.5
    for a in (X, y, xi, g):
        a.setflags(write=False)
    return y, X, (np.zeros(k), np.eye(k) * 10.0, 1.0, 1e-12), xi, g


def floor_hits_on_the_cpu():
    """The iterations of the floor problem whose sigma2 the oracle floors, as booleans [T]."""
    from oracle import bmc_oracle as O
    y, X, prior, xi, g = floor_problem()
    _, trace = O.gibbs_replay(y, np.asarray(X), T_LONG, prior, xi, g, return_sigma2=True)
    return trace[1:] == SIGMA2_FLOOR


def run_floor(ctx):
    """Returns (chain [T, k + 1], stats)."""
    y, X, prior, xi, g = floor_problem()
    ctx.set_problem(y, X)
    ctx.set_prior(*prior)
    ctx.set_tuning(**FLOOR_TUNING)
    try:
        out, st = ctx.gibbs_run(1, T_LONG, xi=xi[None], g=g[None])
    finally:
        ctx.set_tuning()
    lc.check_stats(FLOOR, st, FLOOR_TUNING)
    return out[0], st
