"""Power-scaling sensitivity of a sampled fit on the GPU: does the answer depend on the prior?

The reference package hard-codes its priors (``b_mean_cov = diag(S_hat^2)``, ``nu0 = 1``,
``sigma20 = 0.02``) and has no check of them; this is a capability of this build.  The method is
that of N. Kallioinen, T. Paananen, P.-C. Buerkner, A. Vehtari, "Detecting and diagnosing prior and
likelihood sensitivity with power-scaling", Statistics and Computing 34, 2024 (the R package
``priorsense``): the prior, or the likelihood, is raised to a power alpha near 1, the draws already
taken are importance-reweighted with Pareto smoothing, and the shift of every marginal is measured
with the cumulative Jensen-Shannon distance.

The model is the one the Gibbs sampler draws from: ``y_i ~ N(a_i . beta, sigma^2)``,
``beta ~ N(b0, C0)``, ``sigma^2 ~ Inv-Gamma(nu0 / 2, nu0 sigma20 / 2)``.  Per pooled draw s, with
additive constants dropped,

* ``lp_beta   = -1/2 (beta - b0)' C0^-1 (beta - b0)``
* ``lp_sigma2 = -(nu0 / 2 + 1) log sigma^2 - nu0 sigma20 / (2 sigma^2)``
* ``loglik    = -(N / 2) log 2 pi - N log sigma - sum_i (y_i - a_i . beta)^2 / (2 sigma^2)``

and the components are ``prior = lp_beta + lp_sigma2``, ``likelihood = loglik``, ``prior_beta`` and
``prior_sigma2``.  This is the nominal model: the sampler's ``1e-6`` floors and ridge are not part
of it.  A draw with a non-finite coefficient or without a finite ``sigma > 0`` has no log density
(all three are NaN), and a component with such a draw is NaN throughout and flagged.

Weights of component c at power alpha: ``lw = (alpha - 1) lp_c`` shifted to a largest of 0, Pareto
smoothed exactly as ``psis_loo`` smooths its weights (tail of ``M = min(S // 5, ceil(3 sqrt S))``
draws in ascending ``lw`` with ties in draw order; no fit when ``M < 5`` or the tail is one value:
``pareto_k = inf`` and the raw weights; ``gpdfit`` with the weak prior; truncation at 0), then
``w = exp(lw) / sum exp(lw)``.

Per quantity column (``beta_j``, ``sigma`` and, with ``Vt_hat``, the model weights
``beta . Vt_hat + 1 / M``) and weight vector, with the draws sorted by (value, draw index),
``d_j = x_(j+1) - x_(j)`` (``d_S = 0``), ``P_j = j / S``, ``Q_j = sum_{i <= j} w_(i)``,
``m_j = (P_j + Q_j) / 2``, ``I_P = sum P_j d_j``, ``I_Q = sum Q_j d_j``:

* ``cjs_PQ = max(0, sum d_j P_j log2(P_j / m_j) + (I_Q - I_P) / (2 ln 2))``
* ``cjs_QP = max(0, sum d_j Q_j log2(Q_j / m_j) + (I_P - I_Q) / (2 ln 2))`` (a term with ``Q_j = 0`` is 0)
* ``cjs = sqrt((cjs_PQ + cjs_QP) / (I_P + I_Q))``, 0 for a constant column,

and the weighted mean and sd.  The sensitivity is
``psens = (cjs(alpha_lo) + cjs(alpha_hi)) / (2 log2 alpha_hi)``; at the threshold 0.05, prior and
likelihood both at or above it read ``"prior-data conflict"``, the prior alone
``"strong prior / weak likelihood"``, anything else ``"-"``.

Out of scope: moment matching when ``pareto_k`` is high (k is reported), ``r_eff != 1``, the
simplex sampler (its target is not this posterior), power-scaling parts of the likelihood, plots.
"""
from __future__ import annotations

import numpy as np

from .scoring import _pointwise_call

COMPONENTS = ("prior", "likelihood", "prior_beta", "prior_sigma2")   # the bit order of the C ABI
DEFAULT_COMPONENTS = ("prior", "likelihood")
MAX_ALPHAS = 64
THRESHOLD = 0.05
CONFLICT = "prior-data conflict"
STRONG_PRIOR = "strong prior / weak likelihood"
NO_FINDING = "-"


def _check_alpha(name, a):
    try:
        a = float(a)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number") from None
    if not np.isfinite(a) or a <= 0.0 or a == 1.0:
        raise ValueError(f"{name} must be positive, finite and not 1; got {a}")
    return a


def _check_components(components):
    if isinstance(components, str):
        components = (components,)
    components = tuple(components)
    if not components:
        raise ValueError("components must name at least one of " + ", ".join(COMPONENTS))
    for c in components:
        if c not in COMPONENTS:
            raise ValueError(f"unknown component {c!r}; known: " + ", ".join(COMPONENTS))
    if len(set(components)) != len(components):
        raise ValueError("components must not repeat")
    # the C ABI returns the components in bit order
    return tuple(c for c in COMPONENTS if c in components)


def _check_prior(prior_info, k):
    try:
        b0, C0, nu0, sigma20 = prior_info
    except (TypeError, ValueError):
        raise ValueError("prior_info must be [b0, C0, nu0, sigma20]") from None
    b0 = np.asarray(b0, dtype=np.float64)
    C0 = np.asarray(C0, dtype=np.float64)
    if b0.shape != (k,):
        raise ValueError(f"b0 must be ({k},); got {b0.shape}")
    if C0.shape != (k, k):
        raise ValueError(f"C0 must be ({k}, {k}); got {C0.shape}")
    nu0, sigma20 = float(nu0), float(sigma20)
    if not (np.isfinite(nu0) and nu0 >= 0 and np.isfinite(sigma20) and sigma20 >= 0):
        raise ValueError("nu0 and sigma20 must be finite and >= 0")
    return b0, C0, nu0, sigma20


def _run(A, y, samples, prior_info, Vt_hat, burn, thin, alphas, components, device, cols_per_batch,
         want_weights):
    a_shape = tuple(np.shape(A))
    if len(a_shape) != 2:
        raise ValueError(f"A must be (n_points, k); got {len(a_shape)} dimensions")
    k = a_shape[1]
    prior = _check_prior(prior_info, k)
    if Vt_hat is not None:
        Vt_hat = np.asarray(Vt_hat, dtype=np.float64)
        if Vt_hat.ndim != 2 or Vt_hat.shape[0] != k or Vt_hat.shape[1] < 1:
            raise ValueError(f"Vt_hat must be ({k}, n_models); got {Vt_hat.shape}")
    mask = sum(1 << COMPONENTS.index(c) for c in components)
    return _pointwise_call("power_sensitivity", "power_sensitivity_device", A, y, samples, burn, thin,
                           device, scalars=(prior, Vt_hat, np.asarray(alphas, dtype=np.float64), mask,
                                            int(cols_per_batch), bool(want_weights)))


def column_names(k, n_models=0, models=None):
    """Names of the quantity columns: ``beta_0 .. beta_{k-1}``, ``sigma`` and the model weights
    (``models`` or ``omega_0 ..``)."""
    if models is not None:
        models = [str(m) for m in models]
        if len(models) != n_models:
            raise ValueError(f"models must name the {n_models} columns of Vt_hat; got {len(models)}")
    else:
        models = [f"omega_{m}" for m in range(n_models)]
    return [f"beta_{j}" for j in range(k)] + ["sigma"] + models


def diagnose(psens_prior, psens_likelihood, threshold=THRESHOLD):
    """The reading of one quantity's two sensitivities (module docstring)."""
    if psens_prior >= threshold and psens_likelihood >= threshold:
        return CONFLICT
    if psens_prior >= threshold and psens_likelihood < threshold:
        return STRONG_PRIOR
    return NO_FINDING


def power_scale_sensitivity(A, y, samples, prior_info, Vt_hat=None, burn=0, thin=1, alphas=None,
                            components=DEFAULT_COMPONENTS, device=0, alpha_lo=0.99, alpha_hi=1.01,
                            models=None, cols_per_batch=0):
    """Prior and likelihood sensitivity of every coefficient, of sigma and of every model weight
    (module docstring), from draws already taken.

    ``A``, ``y``, ``samples``, ``burn``, ``thin`` and ``device`` as ``pointwise_log_likelihood``
    (host arrays, or a CUDA torch tensor of draws); all kept draws of all chains are pooled in
    chain order.  ``prior_info = [b0, C0, nu0, sigma20]`` is the ``gibbs_sampler`` argument; ``C0``
    must be symmetric positive definite (``numpy.linalg.LinAlgError`` otherwise).  ``Vt_hat``
    ``(k, n_models)`` adds the model-weight columns; ``models`` names them.  ``alphas`` is an
    optional grid of at most 64 powers whose whole power-scaling sequence is returned from the same
    call; ``components`` selects among ``COMPONENTS``.  ``cols_per_batch`` forces the number of
    columns sorted together (0: as many as the device memory holds; the results do not depend on it).

    Returns a dict: ``columns`` (names), ``components``, ``alphas`` (``alpha_lo``, ``alpha_hi``, then
    the grid), ``psens[component]`` ``(Q,)``, ``diagnosis`` (one string per column; ``"-"``
    unless both ``prior`` and ``likelihood`` were asked for), per component and alpha ``mean``,
    ``sd``, ``cjs`` ``[component] (n_alphas, Q)`` and ``pareto_k[component] (n_alphas,)``, the per-draw
    ``log_prior``, ``log_lik``, ``log_prior_beta``, ``log_prior_sigma2`` ``(S,)``, the boolean
    ``component_flags`` / ``column_flags`` of non-finite input, ``threshold`` and ``n_draws``."""
    components = _check_components(components)
    lo, hi = _check_alpha("alpha_lo", alpha_lo), _check_alpha("alpha_hi", alpha_hi)
    if not lo < 1.0 < hi:
        raise ValueError("need alpha_lo < 1 < alpha_hi")
    grid = [] if alphas is None else [_check_alpha("alpha", a) for a in np.asarray(alphas).reshape(-1)]
    if len(grid) > MAX_ALPHAS:
        raise ValueError(f"at most {MAX_ALPHAS} alphas; got {len(grid)}")
    all_alphas = np.array([lo, hi] + grid, dtype=np.float64)
    out = _run(A, y, samples, prior_info, Vt_hat, burn, thin, all_alphas, components, device,
               cols_per_batch, False)
    k = np.shape(A)[1]
    n_models = 0 if Vt_hat is None else np.shape(Vt_hat)[1]
    res = {"columns": column_names(k, n_models, models), "components": components,
           "alphas": all_alphas, "threshold": THRESHOLD, "n_draws": int(out["logdens"].shape[1]),
           "psens": {}, "mean": {}, "sd": {}, "cjs": {}, "pareto_k": {}}
    for ci, c in enumerate(components):
        for key in ("mean", "sd", "cjs", "pareto_k"):
            res[key][c] = out[key][ci]
        res["psens"][c] = (out["cjs"][ci, 0] + out["cjs"][ci, 1]) / (2.0 * np.log2(hi))
    if "prior" in components and "likelihood" in components:
        res["diagnosis"] = [diagnose(p, l) for p, l in zip(res["psens"]["prior"],
                                                           res["psens"]["likelihood"])]
    else:
        res["diagnosis"] = [NO_FINDING] * len(res["columns"])
    lb, ls, ll = out["logdens"]
    res.update(log_prior=lb + ls, log_lik=ll, log_prior_beta=lb, log_prior_sigma2=ls,
               component_flags=dict(zip(components, out["component_flags"].tolist())),
               column_flags=out["column_flags"])
    return res


def power_scale_weights(A, y, samples, prior_info, component="prior", alpha=1.01, burn=0, thin=1,
                        device=0):
    """The Pareto-smoothed, normalised importance weights of the pooled draws under one component
    raised to the power ``alpha`` (module docstring): what reweights any other function of the
    draws.  Arguments as ``power_scale_sensitivity``.  Returns ``(weights (S,), pareto_k)``;
    ``pareto_k`` is inf where nothing was smoothed, the weights NaN when the component has a
    non-finite log density."""
    (component,) = _check_components((component,) if isinstance(component, str) else component)
    alpha = _check_alpha("alpha", alpha)
    out = _run(A, y, samples, prior_info, None, burn, thin, [alpha], (component,), device, 0, True)
    return out["weights"][:, 0].copy(), float(out["pareto_k"][0, 0])


def sensitivity_summary(result, threshold=THRESHOLD):
    """The table of ``power_scale_sensitivity``'s result: one row per quantity, one column of
    ``psens`` per component and the diagnosis at ``threshold`` (a pandas DataFrame)."""
    import pandas as pd
    threshold = float(threshold)
    if not threshold > 0:
        raise ValueError("threshold must be > 0")
    cols = {c: np.asarray(result["psens"][c]) for c in result["components"]}
    if "prior" in cols and "likelihood" in cols:
        diag = [diagnose(p, l, threshold) for p, l in zip(cols["prior"], cols["likelihood"])]
    else:
        diag = [NO_FINDING] * len(result["columns"])
    cols["diagnosis"] = diag
    return pd.DataFrame(cols, index=list(result["columns"]))
