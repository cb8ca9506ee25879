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

With ``nu=`` the model is the one the robust sampler draws from (``gibbs_sampler_robust``,
``train({"sampler": "student_t"})``): ``y_i ~ a_i . beta + sigma t_nu``, the latent row weights
integrated out as ``scoring`` integrates them.  The priors and ``lp_beta``, ``lp_sigma2`` are the
same; with ``r_i = y_i - a_i . beta``

* ``loglik = N (C(nu) - log sigma) - (nu + 1)/2 sum_i log1p(r_i^2 / (nu sigma^2))``,
  ``C(nu) = lgamma((nu + 1)/2) - lgamma(nu/2) - 1/2 log(nu pi)``.

With ``nu_draws=`` (a fit that estimated ``nu``: ``gibbs_sampler_robust(nu="estimate")``) draw s has
its own ``nu_s`` in place of ``nu``, and ``nu`` is one more quantity column, the last.  That fit has
a prior the others lack, the discrete prior of ``nu``: with ``nu_grid`` / ``nu_prior`` (the
sampler's arguments, through ``robust_nu_prior``)

* ``lp_nu = log(w_g / sum w)`` for ``nu_s = nu_grid[g]``

joins the prior, ``prior = lp_beta + lp_sigma2 + lp_nu``, and is a component of its own,
``prior_nu`` (``T_COMPONENTS``): whether the posterior of ``nu``, and the ``sigma`` and weights that
move with it, only restates that prior.  Without them ``lp_nu = 0``.

Out of scope: moment matching when ``pareto_k`` is high (k is reported), ``r_eff != 1``, the
simplex sampler (its target is not this posterior), power-scaling parts of the likelihood, plots.
"""
from __future__ import annotations

import numpy as np

from .scoring import _check_nu, _is_torch, _nu_table, _pointwise_call

COMPONENTS = ("prior", "likelihood", "prior_beta", "prior_sigma2")   # the bit order of the C ABI
T_COMPONENTS = COMPONENTS + ("prior_nu",)   # of the Student-t forms; prior_nu only with a nu prior
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


def _check_components(components, known=COMPONENTS):
    if isinstance(components, str):
        components = (components,)
    components = tuple(components)
    if not components:
        raise ValueError("components must name at least one of " + ", ".join(known))
    for c in components:
        if c not in known:
            if c in T_COMPONENTS:
                raise ValueError(f"the component {c!r} needs nu_draws and a nu prior (nu_grid, nu_prior)")
            raise ValueError(f"unknown component {c!r}; known: " + ", ".join(known))
    if len(set(components)) != len(components):
        raise ValueError("components must not repeat")
    # the C ABI returns the components in bit order
    return tuple(c for c in known if c in components)


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


def _likelihood(nu, nu_draws, nu_grid, nu_prior, samples, burn, thin):
    """What a call needs of the likelihood: a dict with ``host`` / ``device`` (the context methods),
    ``scalars`` (what they take behind ``want_weights``), ``held`` (kept alive during the call),
    ``known`` (the components it has), ``name`` and ``nu`` (the result's ``likelihood`` and ``nu``)
    and ``nu_column``.  ValueError for what the module docstring rules out (no GPU needed)."""
    if nu_draws is None and (nu_grid is not None or nu_prior is not None):
        raise ValueError("nu_grid and nu_prior describe the prior of nu_draws; give nu_draws")
    name = "power_sensitivity"
    lik = {"host": name, "device": name + "_device", "scalars": (), "held": None, "known": COMPONENTS,
           "name": "gaussian", "nu": None, "nu_column": False}
    if nu_draws is None:
        nu = _check_nu(nu)
        if nu is not None:
            lik.update(host=name + "_t", device=name + "_t_device", scalars=(nu,), name="student_t", nu=nu)
        return lik
    if nu is not None:
        raise ValueError("give nu (one value for all draws) or nu_draws (one per draw), not both")
    values, index = _nu_table(nu_draws, samples, burn, thin)
    held = index
    if _is_torch(samples) and samples.is_cuda:   # the index goes where the draws are
        import torch
        held = torch.as_tensor(index, device=samples.device)
    log_prior = None
    if nu_grid is not None or nu_prior is not None:
        from .inference_utils import robust_nu_prior
        grid, weight, _ = robust_nu_prior(nu_grid, nu_prior)
        at = np.searchsorted(grid, values)
        at[at == grid.shape[0]] = 0
        if not (np.all(grid[at] == values) and np.all(weight[at] > 0)):
            raise ValueError("every value of nu_draws must be a value of nu_grid with a positive prior weight")
        log_prior = np.log(weight[at] / weight.sum())
        lik["known"] = T_COMPONENTS
    lik.update(host=name + "_tv", device=name + "_tv_device", held=held, name="student_t",
               scalars=(values, index if held is index else held.data_ptr(), log_prior),
               nu=float(np.mean(values[index])), nu_column=True)
    return lik


def _run(A, y, samples, prior_info, Vt_hat, burn, thin, alphas, components, device, cols_per_batch,
         want_weights, lik=None):
    a_shape = tuple(np.shape(A))
    if len(a_shape) != 2:
        raise ValueError(f"A must be (n_points, k); got {len(a_shape)} dimensions")
    k = a_shape[1]
    prior = _check_prior(prior_info, k)
    if Vt_hat is not None:
        Vt_hat = np.asarray(Vt_hat, dtype=np.float64)
        if Vt_hat.ndim != 2 or Vt_hat.shape[0] != k or Vt_hat.shape[1] < 1:
            raise ValueError(f"Vt_hat must be ({k}, n_models); got {Vt_hat.shape}")
    mask = sum(1 << T_COMPONENTS.index(c) for c in components)
    host, dev, tail = (("power_sensitivity", "power_sensitivity_device", ()) if lik is None else
                       (lik["host"], lik["device"], lik["scalars"]))
    return _pointwise_call(host, dev, A, y, samples, burn, thin,
                           device, scalars=(prior, Vt_hat, np.asarray(alphas, dtype=np.float64), mask,
                                            int(cols_per_batch), bool(want_weights), *tail))


def column_names(k, n_models=0, models=None, nu=False):
    """Names of the quantity columns: ``beta_0 .. beta_{k-1}``, ``sigma`` and the model weights
    (``models`` or ``omega_0 ..``); with ``nu`` one more, ``nu``, the last."""
    if models is not None:
        models = [str(m) for m in models]
        if len(models) != n_models:
            raise ValueError(f"models must name the {n_models} columns of Vt_hat; got {len(models)}")
    else:
        models = [f"omega_{m}" for m in range(n_models)]
    return [f"beta_{j}" for j in range(k)] + ["sigma"] + models + (["nu"] if nu else [])


def diagnose(psens_prior, psens_likelihood, threshold=THRESHOLD):
    """The reading of one quantity's two sensitivities (module docstring)."""
    if psens_prior >= threshold and psens_likelihood >= threshold:
        return CONFLICT
    if psens_prior >= threshold and psens_likelihood < threshold:
        return STRONG_PRIOR
    return NO_FINDING


def power_scale_sensitivity(A, y, samples, prior_info, Vt_hat=None, burn=0, thin=1, alphas=None,
                            components=DEFAULT_COMPONENTS, device=0, alpha_lo=0.99, alpha_hi=1.01,
                            models=None, cols_per_batch=0, nu=None, nu_draws=None, nu_grid=None,
                            nu_prior=None):
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
    ``component_flags`` / ``column_flags`` of non-finite input, ``threshold`` and ``n_draws``.

    ``nu=None`` is the Gaussian likelihood; a positive finite number the Student-t one with that
    many degrees of freedom.  ``nu_draws`` (instead of ``nu``) is the Student-t likelihood with a
    ``nu`` per draw, as ``pointwise_log_likelihood`` takes it; the columns then end in ``nu``.
    ``nu_grid`` and ``nu_prior`` (only with ``nu_draws``; the arguments of
    ``gibbs_sampler_robust(nu="estimate")``, defaults included when one of the two is given) are
    the prior that fit gave ``nu``: it joins ``prior``, and ``prior_nu`` becomes a component
    (``T_COMPONENTS``); every drawn value must be a grid value of positive weight.  The result
    also carries ``likelihood`` (``"gaussian"`` or ``"student_t"``), ``nu`` (None, the value, or
    the mean over the pooled draws) and ``log_prior_nu`` ``(S,)`` (None for the Gaussian
    likelihood, zeros without a prior of ``nu``)."""
    lik = _likelihood(nu, nu_draws, nu_grid, nu_prior, samples, burn, thin)
    components = _check_components(components, lik["known"])
    lo, hi = _check_alpha("alpha_lo", alpha_lo), _check_alpha("alpha_hi", alpha_hi)
    if not lo < 1.0 < hi:
        raise ValueError("need alpha_lo < 1 < alpha_hi")
    grid = [] if alphas is None else [_check_alpha("alpha", a) for a in np.asarray(alphas).reshape(-1)]
    if len(grid) > MAX_ALPHAS:
        raise ValueError(f"at most {MAX_ALPHAS} alphas; got {len(grid)}")
    all_alphas = np.array([lo, hi] + grid, dtype=np.float64)
    out = _run(A, y, samples, prior_info, Vt_hat, burn, thin, all_alphas, components, device,
               cols_per_batch, False, lik)
    k = np.shape(A)[1]
    n_models = 0 if Vt_hat is None else np.shape(Vt_hat)[1]
    res = {"columns": column_names(k, n_models, models, lik["nu_column"]), "components": components,
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
    lb, ls, ll = out["logdens"][:3]
    ln = out["logdens"][3] if lik["name"] == "student_t" else None
    res.update(log_prior=lb + ls if ln is None else (lb + ls) + ln, log_lik=ll, log_prior_beta=lb,
               log_prior_sigma2=ls, log_prior_nu=ln, likelihood=lik["name"], nu=lik["nu"],
               component_flags=dict(zip(components, out["component_flags"].tolist())),
               column_flags=out["column_flags"])
    return res


def power_scale_weights(A, y, samples, prior_info, component="prior", alpha=1.01, burn=0, thin=1,
                        device=0, nu=None, nu_draws=None, nu_grid=None, nu_prior=None):
    """The Pareto-smoothed, normalised importance weights of the pooled draws under one component
    raised to the power ``alpha`` (module docstring): what reweights any other function of the
    draws.  Arguments as ``power_scale_sensitivity``, the likelihood (``nu``, ``nu_draws``,
    ``nu_grid``, ``nu_prior``) included.  Returns ``(weights (S,), pareto_k)``;
    ``pareto_k`` is inf where nothing was smoothed, the weights NaN when the component has a
    non-finite log density."""
    lik = _likelihood(nu, nu_draws, nu_grid, nu_prior, samples, burn, thin)
    (component,) = _check_components((component,) if isinstance(component, str) else component,
                                     lik["known"])
    alpha = _check_alpha("alpha", alpha)
    out = _run(A, y, samples, prior_info, None, burn, thin, [alpha], (component,), device, 0, True, lik)
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
