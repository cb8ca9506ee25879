"""The cases of tests/test_leader_stream_gpu.py and scripts/record_leader_stream_golden.py: the
smallest launches that reach what the leader wave's loop control touches -- the variate prefetch
past a chain's last row, both parities of the exchange slot, the lanes past K, the abort word, the
gather's flag -- with their inputs.  All Gibbs cases but the device-generator pair run in replay
mode on streams drawn here: the chains are compared with the bits of the commit the goldens were
recorded at, not with the oracle, so any finite streams serve.  One module builds the inputs for
the recorder and for the test, so that a golden and the run compared with it start from the same
bits.

A golden is tests/golden/leader_stream/<name>.npy: ONE chain [T, k + 1] for a one-chain case, the
launch's chains [chains, T, k + 1] for the cases whose chains have streams of their own."""
import functools
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "leader_stream")
T_MAX = 65
BURN_SIMPLEX = 4
T_SIMPLEX = 3
SIMPLEX_STEPSIZE = 0.01
PAIR_SEEDS = (11, 12)

# name: (n, k, tuning keywords, T, what the launch must report)
GIBBS_CASES = {}
for _G in (2, 32):      # T = 1, 2, 3: the padded last prefetch and both slot parities; 65: a long run
    for _T in (1, 2, 3, 65):
        GIBBS_CASES[f"k16_g{_G}_t{_T}"] = (640, 16, dict(groups_per_chain=_G), _T, dict(groups_per_chain=_G))
for _k in (5, 40):      # KMAX 8: no DPP blocks; KMAX 64: lanes 40..63 must draw 0
    for _T in (3, 65):
        GIBBS_CASES[f"k{_k}_g3_t{_T}"] = (640, _k, dict(groups_per_chain=3), _T, dict(groups_per_chain=3))
# the kernel the benchmark measures, in the geometry the planner gives it
GIBBS_CASES["headline_t65"] = (10000, 32, dict(), 65, dict(groups_per_chain=32, waves_per_group=5))
GIBBS_CASES["k16_g3_agent_t3"] = (640, 16, dict(groups_per_chain=3, force_agent_scope=1), 3,
                                  dict(groups_per_chain=3, xcd_local_chains=0))
PAIR_REPLAY, PAIR_DEVICE, PACK16, SIMPLEX_CASE = "pair_replay_t2", "pair_device_t2", "pack16_t3", "simplex_g3_t3"
PAIR_TUNING = dict(groups_per_chain=2)
PACK_TUNING = dict(panels_per_wave=1)
CASES = list(GIBBS_CASES) + [PAIR_REPLAY, PAIR_DEVICE, PACK16, SIMPLEX_CASE]


def golden_path(name):
    return os.path.join(GOLDEN_DIR, name + ".npy")


@functools.lru_cache(maxsize=None)
def problem(n, k):
    """One problem per shape, shared by the cases and never modified."""
    rng = np.random.default_rng(7000 * n + k)
    X = np.asfortranarray(rng.standard_normal((n, k)) / np.sqrt(n))
    y = X @ rng.standard_normal(k) + 0.1 * rng.standard_normal(n)
    for a in (X, y):
        a.setflags(write=False)
    return y, X, (np.zeros(k), np.eye(k) * 10.0, 1.0, 0.02)


@functools.lru_cache(maxsize=None)
def streams(n, k, s=0):
    """(xi [T_MAX, k], g [T_MAX]) of stream number s; a case of T iterations takes the first T rows,
    so the chains of one shape are prefixes of one another."""
    rng = np.random.default_rng([n, k, s])
    xi = rng.standard_normal((T_MAX, k))
    g = rng.standard_gamma((1.0 + n) / 2, size=T_MAX)
    xi.setflags(write=False)
    g.setflags(write=False)
    return xi, g


def load(ctx, n, k):
    y, X, prior = problem(n, k)
    ctx.set_problem(y, X)
    ctx.set_prior(*prior)


def run_replay(ctx, n, k, T, which=(0,)):
    """One launch of len(which) chains, chain c on stream which[c]."""
    xi = np.stack([streams(n, k, s)[0][:T] for s in which])
    g = np.stack([streams(n, k, s)[1][:T] for s in which])
    return ctx.gibbs_run(len(which), T, xi=xi, g=g)


def check_stats(name, st, want):
    for key, v in want.items():
        assert st[key] == v, (name, key, st)
    assert st["groups_per_chain"] > 1, (name, st)      # (a chain in one workgroup has no leader stream)


def run_gibbs_case(ctx, name):
    """Returns (chain [T, k + 1], stats)."""
    n, k, tuning, T, want = GIBBS_CASES[name]
    load(ctx, n, k)
    ctx.set_tuning(**tuning)
    try:
        out, st = run_replay(ctx, n, k, T)
    finally:
        ctx.set_tuning()
    check_stats(name, st, want)
    return out[0], st


def run_pair(ctx, replay):
    """Two chains with streams of their own in one launch of T = 2, and chain 0 alone.  Returns
    (pair [2, 2, 17], alone [2, 17], stats)."""
    load(ctx, 640, 16)
    ctx.set_tuning(**PAIR_TUNING)
    try:
        if replay:
            pair, st = run_replay(ctx, 640, 16, 2, (0, 1))
            alone, st1 = run_replay(ctx, 640, 16, 2, (0,))
        else:
            pair, st = ctx.gibbs_run(2, 2, seeds=list(PAIR_SEEDS))
            alone, st1 = ctx.gibbs_run(1, 2, seeds=[PAIR_SEEDS[0]])
    finally:
        ctx.set_tuning()
    for s in (st, st1):
        check_stats("pair", s, PAIR_TUNING)
    assert st["n_chains"] == 2 and st["launches"] == 1, st
    return pair, alone[0], st


def run_pack16(ctx):
    """16 chains in one launch (two per XCD), chain c on stream c, T = 3.  Returns
    (chains [16, 3, 17], stats)."""
    load(ctx, 640, 16)
    ctx.set_tuning(**PACK_TUNING)
    try:
        out, st = run_replay(ctx, 640, 16, 3, tuple(range(16)))
    finally:
        ctx.set_tuning()
    assert st["n_chains"] == 16 and st["launches"] == 1 and st["groups_per_chain"] > 1, st
    return out, st


def run_simplex_case(ctx):
    """Returns (chain [T_SIMPLEX, k + 1], accepted, uniforms used, stats)."""
    import census_common as cc
    y, X, Vt_hat, S_hat = cc.simplex_problem(640, 2, False, True)
    Z, U, G = cc.simplex_streams(640, 2, 1, BURN_SIMPLEX + T_SIMPLEX)
    ctx.set_problem(y, X)
    ctx.set_tuning(groups_per_chain=3)
    try:
        out, acc, used, st = ctx.simplex_run(Vt_hat, S_hat, T_SIMPLEX, 1.0, 0.02, BURN_SIMPLEX, SIMPLEX_STEPSIZE,
                                             xi=Z, unif=U, g=G, return_stats=True)
    finally:
        ctx.set_tuning()
    assert st["groups_per_chain"] == 3, st
    return out, acc, used, st
