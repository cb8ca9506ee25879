"""The granule exchange under every poll schedule it runs with (-m gpu): the first level with
workgroup-scope and with agent-scope stores, the two-level exchange of chains over more than 32
groups, 16 chains in one launch and a bundle of 8.  On each, the chain must equal the oracle's
replay at the T2 bar of test_gibbs_parity_gpu.py, and must be the same bits whether it runs alone
or beside other chains: a schedule may move when a total is seen, never what is summed.

(The expiry of the bounded spin is not provoked here; that path is the one of every earlier
version of the gather.)
"""
import functools

import numpy as np
import pytest

from gpu_common import gpu_ctx
from oracle import bmc_oracle as O
from pybmc_amd.chains import posterior_summary

pytestmark = pytest.mark.gpu

REL_BAR = 1e-6      # T2: posterior summaries
T = 300


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@functools.lru_cache(maxsize=None)
def problem(n, k):
    """One problem and one oracle chain per shape, shared by the tests and never modified."""
    rng = np.random.default_rng(1000 * n + k)
    X = np.asfortranarray(rng.standard_normal((n, k)) / np.sqrt(n))
    y = X @ rng.standard_normal(k) + 0.1 * rng.standard_normal(n)
    prior = (np.zeros(k), np.eye(k) * 10.0, 1.0, 0.02)
    st = O.chain_setup(y, X, prior)
    Z, G = O.reference_streams(3, 4, T, k, O.gamma_shape(st))
    ref, trace = O.gibbs_replay(y, X, T, prior, Z, G, return_sigma2=True)
    for a in (X, y, G, ref, trace):
        a.setflags(write=False)
    return y, X, prior, st, G, ref, trace


def load(ctx, n, k):
    y, X, prior, st, G, ref, trace = problem(n, k)
    ctx.set_problem(y, X)
    ctx.set_prior(*prior)
    W, lam, _ = ctx.basis()
    xi = O.innovations_in_basis(st, y, X, ref, W, lam, trace)
    return xi, G, ref


def check_t2(out, ref, what):
    err = np.abs(out - ref).max()
    print(f"{what}: max |chain - oracle| = {err:.3e}")
    assert err < 1e-9 * max(1.0, np.abs(ref).max()), what
    a, b = posterior_summary(out, None), posterior_summary(ref, None)
    for key in b:
        assert rel(a[key], b[key]) < REL_BAR, (what, key)


def run(ctx, nch, xi, G):
    return ctx.gibbs_run(nch, T, xi=np.repeat(xi[None], nch, 0), g=np.repeat(G[None], nch, 0))


@pytest.mark.parametrize("n,groups,agent", [(640, 2, 0), (640, 3, 0), (640, 32, 0), (640, 32, 1),
                                            (640, 3, 1), (2560, 40, 0)])
def test_forced_geometry_alone_and_beside_others(n, groups, agent):
    """groups_per_chain forced (2, 3, 32: one level; 40 on N = 2 560: teams and two levels), with
    the scope the placement check finds and with agent scope forced."""
    ctx = gpu_ctx()
    xi, G, ref = load(ctx, n, 16)
    ctx.set_tuning(groups, 0, force_agent_scope=agent)
    alone, st1 = run(ctx, 1, xi, G)
    beside, st = run(ctx, 3, xi, G)
    ctx.set_tuning()
    assert st1["groups_per_chain"] == groups and st["groups_per_chain"] == groups
    if agent:
        assert st1["xcd_local_chains"] == 0 and st["xcd_local_chains"] == 0
    check_t2(alone[0], ref, f"n={n} G={groups} agent={agent}")
    for c in range(3):
        assert np.array_equal(beside[c], alone[0]), (c, st, st1)


@pytest.mark.parametrize("nch,cpp", [(16, None), (12, None), (64, 8)])
def test_many_chains_equal_the_chain_alone(nch, cpp):
    """16 and 12 chains in one launch and bundles of 8 (64 chains) at N = 640.  One panel per wave
    is asked for, which keeps the planner from giving so small a chain a single workgroup: the
    chain then has one group per panel and exchanges.  Every slot replays the oracle chain and is
    the bits of the chain run alone in the same geometry."""
    ctx = gpu_ctx()
    xi, G, ref = load(ctx, 640, 16)
    ctx.set_tuning(panels_per_wave=1)
    many, st = run(ctx, nch, xi, G)
    alone, st1 = run(ctx, 1, xi, G)
    ctx.set_tuning()
    print(f"{nch} chains: {st}")
    assert st["n_chains"] == nch and st["launches"] == 1
    assert st["groups_per_chain"] > 1 and st1["groups_per_chain"] == st["groups_per_chain"]
    if cpp:
        assert st["chains_per_pass"] == cpp
    check_t2(alone[0], ref, "alone")
    check_t2(many[0], ref, f"{nch} chains, slot 0")
    for c in range(nch):
        assert np.array_equal(many[c], alone[0]), (c, st, st1)
