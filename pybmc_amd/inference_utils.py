"""Host-side mirror of the reference's ``pybmc/inference_utils.py`` surface.

``gibbs_sampler`` keeps the reference signature and return layout
(reference inference_utils.py:4-56) and runs on the MI355X through the C ABI.
"""
from __future__ import annotations

import numpy as np

from . import _lib


def _draw_seeds(n):
    """Seeds come from numpy's legacy global stream -- the stream the reference's
    beta draw consumes (inference_utils.py:45) -- so ``np.random.seed(s)`` before a
    call makes a run repeatable (the reference itself is not: its sigma2 draw uses
    an unseeded generator, inference_utils.py:52)."""
    hi = np.random.randint(0, 2 ** 32, size=n, dtype=np.uint64)
    lo = np.random.randint(0, 2 ** 32, size=n, dtype=np.uint64)
    return (hi << np.uint64(32)) | lo


def gibbs_sampler(y, X, iterations, prior_info, *, n_chains=1, seeds=None, device=0,
                  dtype=None, return_stats=False, rss="data", _problem_on_device=False):
    """Gibbs sampling for Bayesian linear regression on the GPU.

    Same arguments and result as the reference (inference_utils.py:4-20):
    ``prior_info = (b_mean_prior, b_mean_cov, nu0, sigma20)``; returns an
    ``(iterations, k+1)`` array whose rows are ``[beta, sigma]`` (the last column is
    sigma, not sigma**2, :54).  Raises ``numpy.linalg.LinAlgError`` where the
    reference's ``inv`` calls do (:22, :26).

    Extensions (keyword-only, defaults preserve the reference behaviour):
    ``n_chains`` > 1 returns ``(n_chains, iterations, k+1)``; ``seeds`` fixes the
    per-chain Philox keys; ``dtype=np.float32`` stores X and y in float32 (sums
    stay float64); ``rss="gram"`` (opt-in, at most 64 columns) takes the residual sum of
    squares of :48-51 from sufficient statistics instead of a pass over the data in every
    iteration -- the same chain up to rounding of that sum, one wave per chain.
    """
    if rss not in ("data", "gram"):
        raise ValueError('rss must be "data" or "gram"')
    b0, C0, nu0, s20 = prior_info
    ctx = _lib.default_context(device)
    with ctx.lock:   # (the per-device context is shared: one caller's sequence at a time)
        if not _problem_on_device:   # orthogonalize(method="device") left (y, X) on the GPU
            ctx.set_problem(y, X, dtype=dtype)
        ctx.set_prior(b0, C0, nu0, s20)
        if seeds is None:
            seeds = _draw_seeds(n_chains)
        if rss == "gram":
            ctx.set_tuning(rss_mode=1)
        try:
            out, stats = ctx.gibbs_run(n_chains, int(iterations), seeds=seeds)
        finally:
            if rss == "gram":
                ctx.set_tuning()
    res = out[0] if n_chains == 1 else out
    return (res, stats) if return_stats else res


ROBUST_MAX_K = 32   # bmc_robust_plan.h
ROBUST_MAX_NU_GRID = 64   # bmc_robust_plan.h


def robust_nu_prior(nu_grid=None, nu_prior=None, nu_init=None):
    """The discrete prior of ``gibbs_sampler_robust(nu="estimate")``: (grid, weights, start index).
    Defaults: ``numpy.geomspace(1, 100, 64)``; the Gamma(shape 2, rate 0.1) density at the grid
    times ``nu_g`` (the quadrature weight of a geometric grid); the grid value nearest 4 among
    those of positive weight.  ``nu_init`` is a value of the grid.  ``ValueError`` for what
    bmc_robust_run_nu refuses."""
    grid = np.geomspace(1.0, 100.0, 64) if nu_grid is None else np.array(nu_grid, dtype=np.float64).reshape(-1)
    if not 1 <= grid.shape[0] <= ROBUST_MAX_NU_GRID:
        raise ValueError(f"nu_grid needs between 1 and {ROBUST_MAX_NU_GRID} values; got {grid.shape[0]}")
    if not (np.all(np.isfinite(grid)) and np.all(grid > 0) and np.all(np.diff(grid) > 0)):
        raise ValueError("nu_grid must be positive, finite and strictly increasing")
    if nu_prior is None:
        weight = grid * (grid * np.exp(-0.1 * grid))
    else:
        weight = np.array(nu_prior, dtype=np.float64).reshape(-1)
        if weight.shape != grid.shape:
            raise ValueError("nu_prior must have one weight per value of nu_grid")
    if not (np.all(np.isfinite(weight)) and np.all(weight >= 0) and np.any(weight > 0)):
        raise ValueError("nu_prior must be non-negative and finite with at least one positive weight")
    if nu_init is None:
        ok = np.flatnonzero(weight > 0)
        init = int(ok[np.argmin(np.abs(grid[ok] - 4.0))])
    else:
        hit = np.flatnonzero(grid == float(nu_init))
        if hit.shape[0] != 1:
            raise ValueError("nu_init must be a value of nu_grid")
        init = int(hit[0])
        if not weight[init] > 0:
            raise ValueError("nu_init must have a positive prior weight")
    return grid, weight, init


def gibbs_sampler_robust(y, X, iterations, prior_info, nu=4.0, *, burn=0, n_chains=1, seeds=None,
                         device=0, return_row_weights=False, return_stats=False, nu_grid=None,
                         nu_prior=None, nu_init=None, return_nu=False):
    """Outlier-robust Gibbs sampling on the GPU (not in the reference): ``gibbs_sampler``'s model
    and priors with a Student-t likelihood ``y_n ~ t_nu(x_n . beta, sigma^2)``, written as a scale
    mixture of normals with one latent weight ``lambda_n ~ Gamma(nu/2, rate nu/2)`` per row.
    ``nu > 0`` is fixed (default 4).  ``prior_info`` is that of ``gibbs_sampler``.

    Every chain runs ``burn + iterations`` sweeps from ``lambda = 1`` and the OLS ``sigma^2`` and
    keeps the last ``iterations``.  Returns ``(iterations, k+1)`` rows ``[beta, sigma]``, or
    ``(n_chains, iterations, k+1)``; with ``return_row_weights`` also the posterior mean of
    ``lambda_n`` over the kept sweeps, ``(N,)`` or ``(n_chains, N)``: a per-row outlier score (about
    1 for a row the model reaches, far below 1 for an outlier).  ``seeds`` fixes the per-chain
    Philox keys; chain c is bit for bit the one-chain run with ``seeds[c]``.  At most 32 columns,
    float64 storage.  ``ValueError`` for ``nu <= 0``, ``burn < 0``, ``n_chains < 1``, a wrong number of
    seeds or more than 32 columns; ``numpy.linalg.LinAlgError`` where ``gibbs_sampler`` raises it, and
    when a chain's conditional precision stops being positive definite.

    ``nu="estimate"`` gives the degrees of freedom a discrete prior and draws them in every sweep
    (an exact categorical draw given the row weights): ``nu_grid`` at most 64 increasing values
    (default ``numpy.geomspace(1, 100, 64)``), ``nu_prior`` their weights (default the Gamma(2, 0.1)
    density times ``nu_g``), ``nu_init`` the starting value (a grid value; default the one nearest
    4).  With ``return_nu`` the draws of ``nu`` -- values, ``(iterations,)`` or ``(n_chains,
    iterations)`` -- follow the row weights in the returned tuple.  A number for ``nu`` keeps it
    fixed; the grid arguments and ``return_nu`` are then refused."""
    estimate = isinstance(nu, str)
    if estimate:
        if nu != "estimate":
            raise ValueError('nu must be a positive number or "estimate"')
        grid, weight, init = robust_nu_prior(nu_grid, nu_prior, nu_init)
    else:
        if nu_grid is not None or nu_prior is not None or nu_init is not None or return_nu:
            raise ValueError('nu_grid, nu_prior, nu_init and return_nu need nu="estimate"')
        nu = float(nu)
        if not nu > 0 or not np.isfinite(nu):
            raise ValueError("nu must be positive and finite")
    if burn < 0:
        raise ValueError("Burn-in iterations must be non-negative.")
    n_chains = int(n_chains)
    if n_chains < 1:
        raise ValueError("n_chains must be >= 1")
    if int(iterations) < 0:
        raise ValueError("iterations must be non-negative")
    if seeds is not None:
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64).reshape(-1)
        if seeds.shape[0] != n_chains:
            raise ValueError(f"seeds has {seeds.shape[0]} entries for n_chains = {n_chains}")
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError("X must be (n, k)")
    if X.shape[1] > ROBUST_MAX_K:
        raise ValueError(f"gibbs_sampler_robust supports at most {ROBUST_MAX_K} columns; "
                         f"got {X.shape[1]}")
    b0, C0, nu0, s20 = prior_info
    ctx = _lib.default_context(device)
    with ctx.lock:
        ctx.set_problem(y, X, dtype=np.float64)
        ctx.set_prior(b0, C0, nu0, s20)
        if seeds is None:
            seeds = _draw_seeds(n_chains)
        if estimate:
            out, w, idx, _, stats = ctx.robust_run(None, n_chains, int(iterations), int(burn), seeds=seeds,
                                                   want_weights=return_row_weights, nu_grid=grid,
                                                   nu_weight=weight, nu_init=init)
        else:
            out, w, stats = ctx.robust_run(nu, n_chains, int(iterations), int(burn), seeds=seeds,
                                           want_weights=return_row_weights)
    res = [out[0] if n_chains == 1 else out]
    if return_row_weights:
        res.append(w[0] if n_chains == 1 else w)
    if return_nu:
        nus = grid[idx]
        res.append(nus[0] if n_chains == 1 else nus)
    if return_stats:
        res.append(stats)
    return res[0] if len(res) == 1 else tuple(res)


def USVt_hat_extraction(U, S, Vt, components_kept):
    """Truncate an SVD to ``components_kept`` components
    (reference inference_utils.py:147-168).  ``U_hat`` is returned column-major
    (F-contiguous), which is also the layout the device kernels read natively."""
    k = int(components_kept)
    U = np.asarray(U)
    S = np.asarray(S)
    Vt = np.asarray(Vt)
    U_hat = np.asfortranarray(U[:, :k])
    S_hat = S[:k]
    Vt_hat_normalized = np.array(Vt[:k])
    Vt_hat = Vt_hat_normalized / S_hat[:, None]
    return U_hat, S_hat, Vt_hat, Vt_hat_normalized


def gibbs_sampler_simplex(y, X, Vt_hat, S_hat, iterations, prior_info, burn=10000,
                          stepsize=0.001, *, seed=None, seeds=None, n_chains=1, device=0,
                          return_stats=False):
    """Random-walk Metropolis on the weight simplex with a Gibbs sigma2 step
    (reference inference_utils.py:59-144).  Same arguments, result, ``ValueError``s
    (:91-94) and acceptance-rate print (:143) as the reference.

    Extensions (keyword-only, defaults preserve the reference behaviour): ``n_chains`` > 1 runs
    that many independent chains side by side on the device and returns ``(n_chains, iterations,
    k+1)``; ``seeds`` (length ``n_chains``) fixes the per-chain Philox keys (``seed`` is the
    one-chain form; giving both is an error), by default they come from numpy's global stream.
    Chain c is bit for bit the one-chain run with ``seed=seeds[c]``.  Every chain starts at
    beta = 0 as the reference does (:82) and ``burn`` is per chain: each chain runs ``burn +
    iterations`` steps and keeps the last ``iterations``.  With several chains the reference's
    line gives the mean acceptance rate and a second line the smallest and largest of the chains.
    """
    if burn < 0:
        raise ValueError("Burn-in iterations must be non-negative.")
    if stepsize <= 0:
        raise ValueError("Stepsize must be positive.")
    n_chains = int(n_chains)
    if n_chains < 1:
        raise ValueError("n_chains must be >= 1")
    if seed is not None and seeds is not None:
        raise ValueError("give seed (one chain) or seeds (one per chain), not both")
    if seeds is not None:
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64).reshape(-1)
        if seeds.shape[0] != n_chains:
            raise ValueError(f"seeds has {seeds.shape[0]} entries for n_chains = {n_chains}")
    elif seed is not None:
        if n_chains != 1:
            raise ValueError("seed names one chain; give seeds (one per chain) with n_chains > 1")
        seeds = np.array([int(seed) & (2 ** 64 - 1)], dtype=np.uint64)
    nu0, s20 = prior_info
    ctx = _lib.default_context(device)
    with ctx.lock:
        ctx.set_problem(y, X)
        if seeds is None:
            seeds = _draw_seeds(n_chains)
        if n_chains == 1:
            samples, accepted, _, stats = ctx.simplex_run(
                Vt_hat, S_hat, int(iterations), float(nu0), float(s20), int(burn), float(stepsize),
                seed=int(seeds[0]), return_stats=True)
        else:
            samples, acc, _, stats = ctx.simplex_run_chains(
                Vt_hat, S_hat, n_chains, int(iterations), float(nu0), float(s20), int(burn),
                float(stepsize), seeds=seeds, return_stats=True)
    if n_chains == 1:
        print(f"Acceptance rate: {accepted / iterations * 100:.2f}%")
    else:
        rates = acc / iterations * 100
        print(f"Acceptance rate: {rates.mean():.2f}%")
        print(f"Acceptance rate per chain: min {rates.min():.2f}%, max {rates.max():.2f}%")
    return (samples, stats) if return_stats else samples
