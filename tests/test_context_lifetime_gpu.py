"""Destroying a context that has run every feature family (-m gpu).

The session's context (gpu_common.gpu_ctx) is never destroyed while the suite runs, so nothing
else exercises bmc_destroy on a context whose buffers are populated: Gibbs, simplex, predict,
diagnostics and the three scoring calls each leave device memory behind.  A second context runs
all of them and is closed; a third one, created afterwards, must then give the session context's
bits.  Shapes are the smallest that still cross a tile edge: 150 rows (three 64-row panels, the
last one partial), 70 points x 130 draws (one full 64-point tile and a remainder, two draw tiles
and a remainder)."""
import numpy as np
import pytest

from conftest import load_golden
from gpu_common import gpu_ctx
from pybmc_amd import _lib

pytestmark = pytest.mark.gpu

CHAINS, ITERS = 2, 40
N_POINTS, N_DRAWS, K_SCORE = 70, 130, 3


def same_bits(a, b):
    """np.array_equal on the raw bytes: NaNs and signed zeros count as values."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return (a.dtype == b.dtype and a.shape == b.shape
            and np.array_equal(a.view(np.uint8), b.view(np.uint8)))


def score_inputs():
    rng = np.random.default_rng(70130)
    A = rng.standard_normal((N_POINTS, K_SCORE))
    beta = np.array([0.5, -0.3, 0.2])
    y = A @ beta + 0.1 * rng.standard_normal(N_POINTS)
    theta = np.column_stack([beta + 0.05 * rng.standard_normal((N_DRAWS, K_SCORE)),
                             rng.uniform(0.08, 0.15, N_DRAWS)])
    return (A, N_POINTS, K_SCORE, K_SCORE, _lib.BMC_ROW_MAJOR, y, theta, N_DRAWS, K_SCORE + 1)


def run_gibbs(ctx):
    g = load_golden("simplex_synth150x4")
    k = g["X"].shape[1]
    ctx.set_problem(g["y"], g["X"])
    ctx.set_prior(np.zeros(k), np.eye(k), float(g["nu0"]), float(g["s20"]))
    return {"gibbs": ctx.gibbs_run(CHAINS, ITERS, seeds=[5, 6])[0]}


def run_loo(ctx):
    return {"loo_" + key: v for key, v in ctx.psis_loo(*score_inputs()).items()}


def run_every_family(ctx):
    out = run_gibbs(ctx)
    k1 = out["gibbs"].shape[2]
    out.update(("diag_" + key, v) for key, v in
               ctx.chain_diagnostics(out["gibbs"], CHAINS, ITERS, k1, k1).items())
    g = load_golden("simplex_synth150x4")
    out["simplex"], out["simplex_accepted"], out["simplex_used"] = ctx.simplex_run_chains(
        g["Vt_hat"], g["S_hat"], CHAINS, ITERS, float(g["nu0"]), float(g["s20"]), int(g["burn"]),
        float(g["stepsize"]), seeds=[7, 8])
    p = load_golden("predict_synth48")
    out["predict_draws"], out["predict_bands"], _ = ctx.predict(p["preds"], p["samples"][:N_DRAWS],
                                                                p["Vt_hat"], seed=3)
    out.update(("score_" + key, v) for key, v in ctx.pointwise_loglik(*score_inputs()).items())
    out.update(run_loo(ctx))
    out.update(("loo_predict_" + key, v) for key, v in ctx.psis_loo_predict(*score_inputs()).items())
    return out


def test_destroying_a_populated_context_leaves_the_next_one_the_same_bits():
    want = run_every_family(gpu_ctx())
    assert want["gibbs"].shape == (CHAINS, ITERS, 5) and want["simplex"].shape == (CHAINS, ITERS, 5)
    assert want["predict_draws"].shape == (N_DRAWS, 48) and want["loo_elpd_loo"].shape == (N_POINTS,)
    assert all(np.isfinite(want[key]).all() for key in ("gibbs", "simplex", "predict_draws",
                                                         "score_lppd", "loo_elpd_loo"))

    second = _lib.Context(0)
    try:
        got = run_every_family(second)
    finally:
        second.close()
    second.close()                      # twice is harmless
    assert second._h is None
    assert sorted(got) == sorted(want)
    for key in want:
        assert same_bits(got[key], want[key]), key

    third = _lib.Context(0)
    try:
        again = {**run_gibbs(third), **run_loo(third)}
    finally:
        third.close()
        third.close()
    assert sorted(again) == ["gibbs", "loo_elpd_loo", "loo_lppd", "loo_pareto_k"]
    for key in again:
        assert same_bits(again[key], want[key]), key
