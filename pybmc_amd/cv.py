"""Exact K-fold and leave-group-out cross-validation on the GPU, every fold in one call.

PSIS-LOO (``pybmc_amd.scoring.psis_loo``) estimates what leaving ONE point out would do, from one
fit, and says where it cannot be trusted (``pareto_k > 0.7``).  The remedy there, and the only way
to ask "what if this whole group had not been measured?", is to refit without the rows in question.
``kfold_cv`` does those refits exactly, all at once.  Rows carry integer labels ``folds[i]`` in
``0 .. F-1``; for every fold f

* the **training rows** are those with ``folds != f``;
* the **posterior** is that of ``gibbs_sampler(y[train], A[train], iterations, prior_info)``: the
  same conditionals, initial sigma^2, gamma shape ``(nu0 + n_train) / 2``, ridge and floors, and
  chain (f, c) consumes the variate streams of ``seeds[f, c]`` -- it is the chain
  ``gibbs_sampler(..., seeds=[seeds[f, c]])`` draws on those rows up to the rounding of its
  residual sums of squares, which come from sufficient statistics (``rss="gram"``);
* the **held-out rows** ``folds == f`` are scored against the S pooled kept draws of fold f (the
  first ``burn`` draws of a chain dropped, every ``thin``-th of the rest kept):
  ``elpd_cv_i = logsumexp_s ll[i, s] - log S`` with ``ll`` of ``pybmc_amd.scoring``, and
  ``cv_mean_i = a_i . mean_s beta_s``.

On the host, in float64: ``elpd_cv = sum_i elpd_cv_i``, ``se = sqrt(n var_i(elpd_cv_i, ddof=1))``,
``cv_rmse = sqrt(mean_i (y_i - cv_mean_i)^2)``, ``elpd_fold[f]`` and ``n_fold[f]``.

On the device (``kernels_cv.hip``): the rows are gathered into fold order once, one pass on the
matrix cores gives the Gram of every fold's own rows, and the training statistics of fold f are the
total minus its own.  The F x C chains then run from those statistics alone, one wave each, in
launches of at most 2048 chains.  At most 64 columns and 1024 folds.

``cv_component_path`` answers "how many components?": the model with k components is the leading k
columns of the same matrix, so one gather and one Gram pass serve every candidate k and all
candidates' chains share the device; ``path_summary`` picks ``k_best`` and, by the
one-standard-error rule, ``k_1se``.
"""
from __future__ import annotations

import numpy as np

from .scoring import _check_int, _check_shapes, _host_matrix, _se, kept_draws

MAX_K = 64
MIN_FOLDS, MAX_FOLDS = 2, 1024


def fold_labels(n, n_folds, seed=None):
    """Balanced random fold labels: a random permutation of ``i % n_folds``, so fold sizes differ by
    at most one.  ``seed`` makes them reproducible (``numpy.random.default_rng(seed)``)."""
    n = _check_int("n", n, 1)
    n_folds = _check_int("n_folds", n_folds, MIN_FOLDS)
    if n_folds > n:
        raise ValueError(f"n_folds = {n_folds} exceeds the number of rows ({n}): a fold would be empty")
    return np.random.default_rng(seed).permutation(np.arange(n, dtype=np.int64) % n_folds)


def group_labels(values):
    """One fold per distinct value (leave-group-out): ``(labels, groups)`` with
    ``groups[labels[i]] == values[i]``, the groups in sorted order."""
    groups, labels = np.unique(np.asarray(values), return_inverse=True)
    return labels.astype(np.int64).reshape(-1), groups


def _check_folds(folds, n, k):
    """int64 labels and F of valid fold labels; ValueError otherwise (no GPU needed)."""
    f = np.asarray(folds)
    if f.shape != (n,):
        raise ValueError(f"folds must be ({n},); got {f.shape}")
    if f.dtype == np.bool_ or not np.issubdtype(f.dtype, np.integer):
        raise ValueError(f"folds must be integer labels; got dtype {f.dtype}")
    f = f.astype(np.int64)
    if f.min() < 0:
        raise ValueError("fold labels must be integers in 0 .. n_folds - 1; got a negative label")
    F = int(f.max()) + 1
    if F < MIN_FOLDS or F > MAX_FOLDS:
        raise ValueError(f"need between {MIN_FOLDS} and {MAX_FOLDS} folds; the labels name {F}")
    count = np.bincount(f, minlength=F)
    if (count == 0).any():
        raise ValueError(f"fold {int(np.argmin(count > 0))} is empty (labels must be 0 .. n_folds - 1, "
                         "every one used)")
    short = np.nonzero(n - count < k)[0]
    if short.size:
        raise ValueError(f"fold {int(short[0])}: its training set has {int(n - count[short[0]])} rows, "
                         f"fewer than k = {k}")
    return f, F, count


def _check_seeds(seed, seeds, F, C):
    from .chains import chain_seeds
    if seeds is not None and seed is not None:
        raise ValueError("give seed or seeds, not both")
    if seeds is None:
        if seed is None:
            from .inference_utils import _draw_seeds
            seed = int(_draw_seeds(1)[0])
        return chain_seeds(int(seed), np.arange(F * C)).reshape(F, C)
    s = np.asarray(seeds)
    if s.shape != (F, C):
        raise ValueError(f"seeds must be (n_folds, n_chains) = ({F}, {C}); got {s.shape}")
    return s.astype(np.uint64)


def cv_summary(y, folds, n_folds, elpd_i, mean_i, n_draws):
    """The host summary of the module docstring from the pointwise vectors (float64)."""
    e = np.asarray(elpd_i, dtype=np.float64)
    m = np.asarray(mean_i, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    return {"elpd_cv": float(np.sum(e)), "se": _se(e),
            "cv_rmse": float(np.sqrt(np.mean((y - m) ** 2))),
            "elpd_fold": np.bincount(folds, weights=e, minlength=n_folds),
            "n_fold": np.bincount(folds, minlength=n_folds), "n_points": int(e.shape[0]),
            "n_folds": int(n_folds), "n_draws": int(n_draws)}


def kfold_cv(A, y, prior_info, folds, iterations, burn=0, thin=1, n_chains=1, seed=None, seeds=None,
             return_draws=False, device=0, nu=None, nu_grid=None, nu_prior=None, nu_init=None,
             return_row_weights=False):
    """Exact cross-validation over the folds named by ``folds`` (module docstring).

    ``A`` is ``(n, k)`` float64 with k <= 64 (either memory order), ``y`` ``(n,)``, ``prior_info =
    [b_mean_prior, b_mean_cov, nu0, sigma20]`` as ``gibbs_sampler`` takes it, ``folds`` ``(n,)``
    integer labels ``0 .. F-1`` (``fold_labels``, ``group_labels``), 2 <= F <= 1024, every label
    used and every training set of at least k rows.  Every fold runs ``n_chains`` chains of
    ``iterations`` iterations; ``seeds`` is ``(F, n_chains)`` uint64, or derived from ``seed`` as
    ``chains.chain_seeds(seed, f * n_chains + c)``, or drawn like ``gibbs_sampler`` draws its own.
    Returns a dict: ``elpd_cv``, ``se``, ``cv_rmse``, ``elpd_fold``, ``n_fold``, ``n_points``,
    ``n_folds``, ``n_draws`` (pooled kept draws per fold), the pointwise ``elpd_cv_i`` and
    ``cv_mean_i``, ``seeds``, and with ``return_draws`` the ``draws`` ``(F, n_chains, kept, k+1)``.
    Argument errors are ``ValueError`` before any GPU work; a fold whose training Gram is
    numerically singular raises ``_lib.SingularFoldError`` naming it.

    ``nu`` selects the Student-t likelihood of ``gibbs_sampler_robust`` (``None``: the Gaussian call
    above, unchanged): a positive number, or ``"estimate"`` with ``nu_grid``, ``nu_prior`` and
    ``nu_init`` as that sampler takes them.  Then k <= 32, and chain (f, c) IS the chain
    ``gibbs_sampler_robust(y[train], A[train], iterations, prior_info, nu, seeds=[seeds[f, c]])``
    draws, bit for bit -- start value, gamma shape and the grid's constants are the training set's
    own -- of which rows ``burn::thin`` are kept; the held-out rows are scored under the t density
    (``scoring.pointwise_log_likelihood(nu=...)``, or ``nu_draws=`` the fold's own draws of nu).
    All F x n_chains chains share one launch, a workgroup each.  The result also carries
    ``likelihood="student_t"`` and ``nu`` (the value, or the pooled mean of the kept draws of nu);
    with ``"estimate"`` and ``return_draws`` the ``nu_draws`` ``(F, n_chains, kept)``; with
    ``return_row_weights`` the ``row_weights`` ``(F, n_chains, n)``: the mean weight of every
    training row over the sweeps after ``burn``, NaN at the fold's own held-out rows.  A chain whose
    conditional precision stops being positive definite raises ``_lib.SingularFoldError`` too."""
    from . import _lib

    A = np.asarray(A)
    y = np.asarray(y)
    if A.dtype != np.float64 or y.dtype != np.float64:
        raise ValueError("A and y must be float64")
    iterations = _check_int("iterations", iterations, 1)
    n_chains = _check_int("n_chains", n_chains, 1)
    # (the draws this call will make, as the shape of samples scoring checks)
    k1 = (A.shape[1] if A.ndim == 2 else 0) + 1
    n, k, C, T, kept = _check_shapes(A.shape, y.shape, (n_chains, iterations, k1), burn, thin)
    grid = weight = init = None
    if nu is None:
        if nu_grid is not None or nu_prior is not None or nu_init is not None or return_row_weights:
            raise ValueError('nu_grid, nu_prior, nu_init and return_row_weights need nu (a number or "estimate")')
    else:
        from .inference_utils import ROBUST_MAX_K, robust_nu_prior
        if isinstance(nu, str):
            if nu != "estimate":
                raise ValueError('nu must be a positive number or "estimate"')
            grid, weight, init = robust_nu_prior(nu_grid, nu_prior, nu_init)
        else:
            if nu_grid is not None or nu_prior is not None or nu_init is not None:
                raise ValueError('nu_grid, nu_prior and nu_init need nu="estimate"')
            nu = float(nu)
            if not nu > 0 or not np.isfinite(nu):
                raise ValueError("nu must be positive and finite")
        if k > ROBUST_MAX_K:
            raise ValueError(f"the Student-t cross-validation supports at most {ROBUST_MAX_K} columns; got {k}")
    if k > MAX_K:
        raise ValueError(f"k must be at most {MAX_K} (one lane per coefficient); got {k}")
    if burn >= iterations:
        raise ValueError(f"burn = {burn} leaves no draw of {iterations} iterations")
    f, F, count = _check_folds(folds, n, k)
    b0, C0, nu0, s20 = prior_info
    b0 = np.asarray(b0, dtype=np.float64)
    C0 = np.asarray(C0, dtype=np.float64)
    if b0.shape != (k,) or C0.shape != (k, k):
        raise ValueError(f"prior_info must hold b_mean_prior ({k},) and b_mean_cov ({k}, {k})")
    seeds = _check_seeds(seed, seeds, F, C)
    Ah, lda, layout = _host_matrix(A)
    ctx = _lib.default_context(device)
    if nu is not None:
        want_idx = grid is not None
        with ctx.lock:
            elpd_i, mean_i, draws, w, idx = ctx.kfold_cv_t(
                Ah, n, k, lda, layout, np.ascontiguousarray(y), f, F, b0, C0, nu0, s20, C, T, int(burn),
                int(thin), seeds.reshape(-1), nu=None if want_idx else nu, nu_grid=grid, nu_weight=weight,
                nu_init=init, return_draws=return_draws, return_row_weights=return_row_weights)
        out = cv_summary(y, f, F, elpd_i, mean_i, C * kept)
        out.update(elpd_cv_i=elpd_i, cv_mean_i=mean_i, seeds=seeds, likelihood="student_t",
                   nu=float(np.mean(grid[idx])) if want_idx else nu)
        if return_draws:
            out["draws"] = draws
            if want_idx:
                out["nu_draws"] = grid[idx]
        if return_row_weights:
            out["row_weights"] = w
        return out
    with ctx.lock:
        elpd_i, mean_i, draws = ctx.kfold_cv(Ah, n, k, lda, layout, np.ascontiguousarray(y), f, F, b0,
                                             C0, nu0, s20, C, T, int(burn), int(thin), seeds.reshape(-1),
                                             return_draws=return_draws)
    out = cv_summary(y, f, F, elpd_i, mean_i, C * kept)
    out.update(elpd_cv_i=elpd_i, cv_mean_i=mean_i, seeds=seeds)
    if return_draws:
        out["draws"] = draws
    return out


def _check_components(components, k_max):
    """int32 candidates of a valid ``components`` (None: 1 .. k_max); ValueError otherwise."""
    if components is None:
        return np.arange(1, k_max + 1, dtype=np.int32)
    try:
        items = list(components)
    except TypeError:
        raise ValueError("components must be a sequence of integers") from None
    if not items:
        raise ValueError("components must name at least one candidate")
    for v in items:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"components must be integers; got {v!r}")
        if v < 1 or v > k_max:
            raise ValueError(f"components must lie in 1 .. {k_max}; got {int(v)}")
    if any(b <= a for a, b in zip(items, items[1:])):
        raise ValueError("components must be strictly increasing, without repeats")
    return np.asarray(items, dtype=np.int32)


def path_summary(components, elpd_cv_i):
    """Which candidate?  ``components`` ``(m,)`` and the pointwise ``elpd_cv_i`` ``(m, n)`` of the
    same rows under every candidate give

    * ``k_best``: the candidate of largest ``elpd_cv`` (the smallest such on a tie);
    * ``elpd_diff[j] = elpd_cv[best] - elpd_cv[j]``;
    * ``se_diff[j] = sqrt(n var_i(elpd_cv_i[best] - elpd_cv_i[j], ddof=1))``, the paired standard
      error of that difference (0 at ``best``);
    * ``k_1se``: the smallest candidate with ``elpd_diff[j] <= se_diff[j]`` -- the
      one-standard-error rule: the most parsimonious model indistinguishable from the best.

    Host, float64; no GPU."""
    comps = np.asarray(components)
    e = np.asarray(elpd_cv_i, dtype=np.float64)
    if comps.ndim != 1 or e.ndim != 2 or e.shape[0] != comps.shape[0] or comps.shape[0] < 1:
        raise ValueError(f"need components (m,) and elpd_cv_i (m, n); got {comps.shape} and {e.shape}")
    elpd = e.sum(axis=1)
    best = int(np.argmax(elpd))          # (the first of equal maxima: the smallest candidate)
    elpd_diff = elpd[best] - elpd
    se_diff = np.array([_se(e[best] - e[j]) if j != best else 0.0 for j in range(e.shape[0])])
    within = np.nonzero(elpd_diff <= se_diff)[0]
    return {"k_best": int(comps[best]), "k_1se": int(comps[within.min()]), "elpd_diff": elpd_diff,
            "se_diff": se_diff}


def cv_component_path(A, y, prior_info, folds, iterations, components=None, burn=0, thin=1, n_chains=1,
                      seed=None, seeds=None, return_draws=False, device=0):
    """``kfold_cv`` for every candidate component count in one call.

    ``A`` is ``(n, k_max)`` float64 with k_max <= 64 (either memory order); ``components`` a
    strictly increasing sequence of integers in ``1 .. k_max`` (default: all of them).  Candidate k
    is the model with design ``A[:, :k]`` and prior ``[b0[:k], C0[:k, :k], nu0, sigma20]`` -- the
    exact marginal of the Gaussian prior.  ``y``, ``prior_info``, ``folds``, ``iterations``,
    ``burn``, ``thin`` and ``n_chains`` as in ``kfold_cv``; every training set must hold at least
    ``max(components)`` rows.  ``seeds`` ``(F, n_chains)`` (or derived from ``seed`` as ``kfold_cv``
    derives them) serve every candidate: chain (k, f, c) consumes the streams of ``seeds[f, c]``
    exactly as ``kfold_cv(A[:, :k], ..., seeds=seeds)`` does, and the result of candidate k is that
    call's.

    Returns a dict, m = ``len(components)``: ``components`` ``(m,)``; ``elpd_cv``, ``se``,
    ``cv_rmse`` ``(m,)`` and ``elpd_fold`` ``(m, F)``; ``n_fold``, ``n_points``, ``n_folds``,
    ``n_draws``; the pointwise ``elpd_cv_i`` and ``cv_mean_i`` ``(m, n)``; ``seeds``; with
    ``return_draws`` ``draws``, a list of m arrays ``(F, n_chains, kept, k + 1)``; and the selection
    of ``path_summary``: ``k_best``, ``k_1se``, ``elpd_diff``, ``se_diff``.  Argument errors are
    ``ValueError`` before any GPU work; a (candidate, fold) whose training Gram is numerically
    singular raises ``_lib.SingularFoldError`` naming the fold and the component count."""
    from . import _lib

    A = np.asarray(A)
    y = np.asarray(y)
    if A.dtype != np.float64 or y.dtype != np.float64:
        raise ValueError("A and y must be float64")
    if A.ndim == 2 and A.shape[1] > MAX_K:
        raise ValueError(f"k_max must be at most {MAX_K} (one lane per coefficient); got {A.shape[1]}")
    iterations = _check_int("iterations", iterations, 1)
    n_chains = _check_int("n_chains", n_chains, 1)
    k1 = (A.shape[1] if A.ndim == 2 else 0) + 1
    n, k_max, C, T, kept = _check_shapes(A.shape, y.shape, (n_chains, iterations, k1), burn, thin)
    if burn >= iterations:
        raise ValueError(f"burn = {burn} leaves no draw of {iterations} iterations")
    comps = _check_components(components, k_max)
    f, F, count = _check_folds(folds, n, int(comps[-1]))
    b0, C0, nu0, s20 = prior_info
    b0 = np.asarray(b0, dtype=np.float64)
    C0 = np.asarray(C0, dtype=np.float64)
    if b0.shape != (k_max,) or C0.shape != (k_max, k_max):
        raise ValueError(f"prior_info must hold b_mean_prior ({k_max},) and b_mean_cov ({k_max}, {k_max})")
    seeds = _check_seeds(seed, seeds, F, C)
    Ah, lda, layout = _host_matrix(A)
    ctx = _lib.default_context(device)
    with ctx.lock:
        elpd_i, mean_i, draws = ctx.cv_path(Ah, n, k_max, lda, layout, np.ascontiguousarray(y), f, F, b0,
                                            C0, nu0, s20, C, T, int(burn), int(thin), seeds.reshape(-1),
                                            comps, return_draws=return_draws)
    per = [cv_summary(y, f, F, elpd_i[j], mean_i[j], C * kept) for j in range(len(comps))]
    out = {"components": comps.astype(np.int64)}
    for key in ("elpd_cv", "se", "cv_rmse", "elpd_fold"):
        out[key] = np.array([p[key] for p in per])
    for key in ("n_fold", "n_points", "n_folds", "n_draws"):
        out[key] = per[0][key]
    out.update(elpd_cv_i=elpd_i, cv_mean_i=mean_i, seeds=seeds)
    if return_draws:
        out["draws"] = draws
    out.update(path_summary(out["components"], elpd_i))
    return out
