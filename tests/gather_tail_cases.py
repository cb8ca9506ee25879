"""The cases of tests/test_gather_tail_gpu.py and scripts/record_gather_tail_golden.py: the smallest
launches that reach every call of the granule gather (bmc_loop.h, exchange_sum), with their inputs.
The Gibbs cases run the problem and the oracle streams of test_exchange_poll_gpu.py in replay mode;
the simplex case runs a problem of census_common.py in replay mode.  One module builds the inputs for
the recorder and for the test, so that a golden and the run compared with it start from the same bits.

Each golden is ONE chain, tests/golden/gather_tail/<name>.npy: all chains of a many-chain case get
the same streams, so every slot must be that chain."""
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gather_tail")
T = 300
BURN_SIMPLEX = 100
SIMPLEX_STEPSIZE = 0.01

# name: (n, tuning keywords, chains in the launch, what the launch must report)
GIBBS_CASES = {
    # first level, the scope the placement check finds (workgroup scope where the groups share an XCD)
    "first_g2": (640, dict(groups_per_chain=2), 1, dict(groups_per_chain=2)),
    "first_g3": (640, dict(groups_per_chain=3), 1, dict(groups_per_chain=3)),
    "first_g32": (640, dict(groups_per_chain=32), 1, dict(groups_per_chain=32)),
    # first level, agent scope forced
    "first_g3_agent": (640, dict(groups_per_chain=3, force_agent_scope=1), 1,
                       dict(groups_per_chain=3, xcd_local_chains=0)),
    "first_g32_agent": (640, dict(groups_per_chain=32, force_agent_scope=1), 1,
                        dict(groups_per_chain=32, xcd_local_chains=0)),
    # more than 32 groups: team totals and the second level
    "teams_g40": (2560, dict(groups_per_chain=40), 1, dict(groups_per_chain=40)),
    # one panel per wave: 16 chains in one launch (two chains per XCD), and 64 chains as bundles of 8
    "pack16": (640, dict(panels_per_wave=1), 16, dict(n_chains=16, launches=1)),
    "bundle64": (640, dict(panels_per_wave=1), 64, dict(n_chains=64, launches=1, chains_per_pass=8)),
}
SIMPLEX_CASE = "simplex_g3"      # 640 rows, 4 models, the workgroup form over 3 groups
CASES = list(GIBBS_CASES) + [SIMPLEX_CASE]


def golden_path(name):
    return os.path.join(GOLDEN_DIR, name + ".npy")


def run_gibbs_case(ctx, name):
    """Returns (chains [n_chains, T, k + 1] of the case, the same chain run alone in that geometry
    or None for a one-chain case, stats)."""
    from test_exchange_poll_gpu import load, run
    n, tuning, nch, want = GIBBS_CASES[name]
    xi, G, _ = load(ctx, n, 16)
    ctx.set_tuning(**tuning)
    try:
        out, st = run(ctx, nch, xi, G)
        alone = run(ctx, 1, xi, G)[0] if nch > 1 else None
    finally:
        ctx.set_tuning()
    for key, v in want.items():
        assert st[key] == v, (name, key, st)
    assert st["groups_per_chain"] > 1, (name, st)      # (a chain in one workgroup gathers nothing)
    return out, alone, st


def simplex_inputs():
    import census_common as cc
    y, X, Vt_hat, S_hat = cc.simplex_problem(640, 2, False, True)
    assert Vt_hat.shape == (2, 4)
    Z, U, G = cc.simplex_streams(640, 2, 1, BURN_SIMPLEX + T)
    return y, X, Vt_hat, S_hat, Z, U, G


def run_simplex_case(ctx):
    """Returns (chain [T, k + 1], accepted, uniforms used, stats)."""
    y, X, Vt_hat, S_hat, Z, U, G = simplex_inputs()
    ctx.set_problem(y, X)
    ctx.set_tuning(groups_per_chain=3)
    try:
        out, acc, used, st = ctx.simplex_run(Vt_hat, S_hat, T, 1.0, 0.02, BURN_SIMPLEX, SIMPLEX_STEPSIZE,
                                             xi=Z, unif=U, g=G, return_stats=True)
    finally:
        ctx.set_tuning()
    assert st["groups_per_chain"] == 3, st
    return out, acc, used, st
