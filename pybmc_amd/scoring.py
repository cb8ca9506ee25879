"""Scoring a sampled fit on the GPU: pointwise log predictive density, WAIC, PSIS-LOO and the
leave-one-out predictive mean, sd and PIT of every training point.

The reference package has no numeric score of a fit; this is a capability of this build.  The
model is the one the samplers draw from, ``y_i ~ N(a_i . beta, sigma^2)``.  For design rows ``A``
(n x k), targets ``y`` and S posterior draws ``(beta_s, sigma_s)``:

    ll[i, s] = -1/2 log(2 pi) - log sigma_s - (y_i - a_i . beta_s)^2 / (2 sigma_s^2)

* ``lppd_i    = logsumexp_s(ll[i, s]) - log S``   (log pointwise predictive density)
* ``p_waic_i  = var_s(ll[i, s])``, ddof 1          (Gelman, Hwang & Vehtari 2014, eq. 12; ``loo::waic``)
* ``mean_ll_i = mean_s(ll[i, s])``

and, on the host in float64 from the pointwise vectors,

* ``elpd_waic_i = lppd_i - p_waic_i``, ``elpd_waic = sum_i``, ``p_waic = sum_i p_waic_i``,
  ``waic = -2 elpd_waic``, ``se = sqrt(n var_i(elpd_waic_i, ddof=1))``,
  ``n_high_p = #{i : p_waic_i > 0.4}`` (the ``loo`` package's warning threshold);
* for held-out data there is no penalty: ``elpd = sum_i lppd_i``, ``se`` from ``lppd_i``.

With ``nu=`` the same estimators score a Student-t fit (``gibbs_sampler_robust``,
``train({"sampler": "student_t"})``): ``y_i ~ a_i . beta + sigma t_nu`` with ``nu`` fixed, and, for
``r = y_i - a_i . beta_s``,

    ll[i, s] = lgamma((nu + 1)/2) - lgamma(nu/2) - 1/2 log(nu pi) - log sigma_s
               - (nu + 1)/2 log1p(r^2 / (nu sigma_s^2))

the marginal t density, the latent row weights integrated out: what leave-one-out needs, since the
``(beta, sigma)`` rows that sampler returns are draws from that marginal posterior.  Everything
downstream of ``ll`` is unchanged.  With ``nu_draws=`` (a fit that estimated ``nu``:
``gibbs_sampler_robust(nu="estimate")``) draw s has its own ``nu_s`` in place of ``nu``.
``compare_elpd`` puts the scores of several fits of the same
data side by side with the paired standard error of their differences.

S. Watanabe, "Asymptotic equivalence of Bayes cross validation and widely applicable information
criterion in singular learning theory", JMLR 11, 2010; A. Gelman, J. Hwang, A. Vehtari,
"Understanding predictive information criteria for Bayesian models", Stat. Comput. 24, 2014.

PSIS-LOO (``psis_loo``; A. Vehtari, A. Gelman, J. Gabry, "Practical Bayesian model evaluation using
leave-one-out cross-validation and WAIC", Stat. Comput. 27, 2017; A. Vehtari, D. Simpson,
A. Gelman, Y. Yao, J. Gabry, "Pareto smoothed importance sampling", JMLR 25, 2024).  Per point i,
over the S pooled kept draws, with r_eff = 1:

1. ``lw_s = -ll[i, s]``, shifted so that the largest is 0 (``c`` the shift);
2. ``M = min(floor(S / 5), ceil(3 sqrt(S)))``; ``M < 5``: nothing is smoothed, ``pareto_k = +inf``;
3. the tail is the M largest ``lw`` (ties by value), ``cutoff`` the largest below it; a tail of equal
   values: nothing is smoothed, ``pareto_k = +inf``;
4. a generalised Pareto distribution is fitted to ``exp(lw_(j)) - exp(cutoff)`` (J. Zhang,
   M. A. Stephens, "A new and efficient estimation method for the generalized Pareto
   distribution", Technometrics 51, 2009, as ``loo::gpdfit``: 30 + floor(sqrt(M)) grid points,
   prior 3, then ``k = (M k + 5) / (M + 10)``); ``pareto_k = k``; a non-finite k: no smoothing;
5. the tail is replaced in rank order by ``log(exp(cutoff) + sigma expm1(-k log1p(-p_j)) / k)``,
   ``p_j = (j - 1/2) / M``, and every ``lw`` truncated at 0;
6. ``elpd_loo_i = logsumexp_s(ll + lw) - logsumexp_s(lw)``, ``p_loo_i = lppd_i - elpd_loo_i``;

and on the host ``elpd_loo = sum_i``, ``p_loo = sum_i``, ``looic = -2 elpd_loo``,
``se = sqrt(n var_i(elpd_loo_i, ddof=1))``, ``n_high_k = #{i : pareto_k_i > 0.7}``,
``k_threshold = min(1 - 1 / log10(S), 0.7)`` and ``n_above_threshold``.

The leave-one-out predictive distribution (``psis_loo_predict``).  Steps 1-5 give every draw an
unnormalised weight ``W_s = exp(lw_s)`` (smoothed for the M tail ranks, raw elsewhere, truncated at
0; raw throughout where nothing is smoothed).  Ties share: draws of point i with equal ``ll[i, s]``
each get the arithmetic mean of the ``W`` of the ranks their run occupies (a run may straddle the
cutoff), so ``sum W`` and ``sum W exp(ll)`` -- ``elpd_loo_i``, ``pareto_k`` -- are unchanged and
every output is a function of the draws' values alone.  With ``w_s = W_s / sum_t W_t``,
``mu_s = a_i . beta_s`` and ``r_s = y_i - mu_s``:

* ``loo_mean_i = y_i - sum_s w_s r_s`` (in the space of ``A`` and ``y``);
* ``loo_sd_i   = sqrt(sum_s w_s (sigma_s^2 + r_s^2) - (sum_s w_s r_s)^2)``;
* ``loo_pit_i  = sum_s w_s Phi(r_s / sigma_s)``, ``Phi(z) = erfc(-z / sqrt 2) / 2``: the
  leave-one-out predictive probability of a value at or below the observed one;
* ``ess_i      = 1 / sum_s w_s^2``, the PSIS effective sample size with r_eff = 1 (1 .. S);

a point with a non-finite ``ll`` gets NaN in each.  Under the Student-t likelihood (``nu=`` or
``nu_draws=``; ``nu_s = nu`` for a fixed one) the weights, the tie sharing, ``ess``, the NaN rules
and the draw limit are these, ``ll`` is the marginal t density above, ``elpd_loo_i``, ``pareto_k``
and ``lppd`` are bit-equal to ``psis_loo`` under the same likelihood arguments, and with
``z_s = r_s / sigma_s``:

* ``loo_mean_i = y_i - sum_s w_s r_s``: the location of the predictive distribution, which is its
  mean where ``nu > 1`` (a t distribution with ``nu <= 1`` has none);
* ``loo_sd_i   = sqrt(sum_s w_s (sigma_s^2 nu_s / (nu_s - 2) + r_s^2) - (sum_s w_s r_s)^2)`` when
  every scored ``nu_s > 2``; ``+inf`` at every point with finite ``ll`` when any scored value
  (``nu``, or any distinct value of the kept ``nu_draws``) is at most 2 -- decided on the host, so
  the device never sums an infinity (a far draw's weight underflows to 0, and ``0 inf`` is NaN);
* ``loo_pit_i  = sum_s w_s F_{nu_s}(z_s)``, ``F_nu`` the Student-t distribution function
  (``student_t_cdf`` of ``bmc_math.h``: the incomplete beta function's continued fraction with the
  density as its prefactor; within 64 times the error of ``scipy.special.stdtr`` for
  ``0.06 <= nu <= 1000``, the range the call accepts);

two more passes over the matrix than ``psis_loo`` (the append runs in two phases: the t density
and distribution function do not fit the registers of one).  On the host ``loo_rmse =
sqrt(mean_i (y_i - loo_mean_i)^2)``, ``pit_coverage[j]`` = the percentage of points with
``|2 loo_pit_i - 1| <= p_j / 100`` for ``p = 0, 5, .., 100`` (the levels and units of
``BayesianModelCombination.evaluate``) and ``min_ess``.  At most 1 863 225 pooled draws.

On the device (``kernels_waic.hip``, ``kernels_loo.hip``) the n x S matrix is never stored: an f64 MFMA GEMM whose
tiles are reduced in the epilogue; PSIS-LOO recomputes it for an exact radix select of each
point's tail.  Non-finite input gives NaN outputs, not an error.
"""
from __future__ import annotations

import numpy as np

POINTWISE_KEYS = ("lppd", "p_waic", "mean_ll")
HIGH_P_WAIC = 0.4
HIGH_PARETO_K = 0.7
MAX_K = 256


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def _check_int(name, v, lo):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
        raise ValueError(f"{name} must be an integer >= {lo}")
    return int(v)


def kept_draws(T, burn, thin):
    """Draws each chain keeps: every ``thin``-th of the ``T - burn`` after the first ``burn``."""
    return max(0, -(-(T - burn) // thin))


def _check_shapes(a_shape, y_shape, s_shape, burn, thin, min_points=1):
    """(n, k, C, T, kept per chain) of valid arguments; ValueError otherwise (no GPU needed)."""
    burn = _check_int("burn", burn, 0)
    thin = _check_int("thin", thin, 1)
    if len(a_shape) != 2:
        raise ValueError(f"A must be (n_points, k); got {len(a_shape)} dimensions")
    n, k = a_shape
    if n < 1:
        raise ValueError("A must hold at least one point")
    if n < min_points:
        raise ValueError(f"A must hold at least {min_points} points; got {n}")
    if k < 1 or k > MAX_K:
        raise ValueError(f"k must be between 1 and {MAX_K}; got {k}")
    if tuple(y_shape) != (n,):
        raise ValueError(f"y must be ({n},); got {tuple(y_shape)}")
    if len(s_shape) not in (2, 3):
        raise ValueError(f"samples must be (T, k+1) or (C, T, k+1); got {len(s_shape)} dimensions")
    C, T, k1 = (1, *s_shape) if len(s_shape) == 2 else tuple(s_shape)
    if k1 != k + 1:
        raise ValueError(f"samples must have k + 1 = {k + 1} columns (coefficients, then sigma); "
                         f"got {k1}")
    if C < 1:
        raise ValueError("samples must hold at least one chain")
    kept = kept_draws(T, burn, thin)
    if C * kept < 2:
        raise ValueError(f"need at least 2 draws after burn and thin (chains = {C}, T = {T}, "
                         f"burn = {burn}, thin = {thin})")
    return n, k, C, T, kept


def _host_matrix(A):
    """(array, lda, layout) of a float64 host matrix, read in place when it is one of the two
    layouts with a contiguous minor dimension."""
    from ._lib import BMC_COL_MAJOR, BMC_ROW_MAJOR
    n, k = A.shape
    st = A.strides
    if st[0] == 8 and st[1] % 8 == 0 and st[1] >= 8 * n:
        return A, st[1] // 8, BMC_COL_MAJOR
    if st[1] == 8 and st[0] % 8 == 0 and st[0] >= 8 * k:
        return A, st[0] // 8, BMC_ROW_MAJOR
    A = np.ascontiguousarray(A)
    return A, k, BMC_ROW_MAJOR


def _point_vectors(vectors, n):
    """The extra per-point vectors of ``_pointwise_call``: each None or float64 ``(n,)``."""
    out = []
    for name, v in vectors:
        if v is not None:
            v = np.asarray(v)
            if v.dtype != np.float64:
                raise ValueError(f"{name} must be float64; got {v.dtype}")
            if v.shape != (n,):
                raise ValueError(f"{name} must be ({n},); got {v.shape}")
            v = np.ascontiguousarray(v)
        out.append(v)
    return out


def _pointwise_call(host_call, device_call, A, y, samples, burn, thin, device, min_points=1,
                    vectors=(), scalars=()):
    """The argument handling the scoring calls and the posterior predictive check share: checks,
    burn / thin / pooling in place where the strides allow it, then the context method named
    ``host_call`` (numpy draws) or ``device_call`` (CUDA tensor draws).  ``vectors`` are further
    ``(name, array or None)`` per-point inputs, checked like ``y`` and handed over after the
    common arguments as host arrays or device addresses; ``scalars`` follow them, either plain
    values or functions of the checked ``(A, y, *vectors)``."""
    from . import _lib

    def tail(A, y, vecs):
        return [f(A, y, *vecs) if callable(f) else f for f in scalars]

    if _is_torch(samples) and not samples.is_cuda:
        samples = samples.numpy()
    A = np.asarray(A)
    y = np.asarray(y)
    if A.dtype != np.float64 or y.dtype != np.float64:
        raise ValueError("A and y must be float64")
    if _is_torch(samples):
        import torch
        if samples.dtype != torch.float64:
            raise ValueError(f"samples must be float64; got {samples.dtype}")
        n, k, C, T, kept = _check_shapes(A.shape, y.shape, tuple(samples.shape), burn, thin,
                                         min_points)
        vecs = _point_vectors(vectors, n)
        t = samples if samples.dim() == 3 else samples.unsqueeze(0)
        if t.stride(2) != 1 or t.stride(1) < k + 1:
            raise ValueError("a device tensor must have a contiguous last dimension")
        t = t[:, burn::thin]
        ld = t.stride(1)
        if C > 1 and t.stride(0) != kept * ld:
            t = t.contiguous()   # chains not one strided run of rows: gather the kept draws
            ld = k + 1
        dev = t.device
        ctx = _lib.default_context(dev.index if dev.index is not None else device)
        Ad = torch.as_tensor(np.ascontiguousarray(A), device=dev)
        yd = torch.as_tensor(np.ascontiguousarray(y), device=dev)
        vd = [None if v is None else torch.as_tensor(v, device=dev) for v in vecs]
        # the library reads on its own stream: what torch queued (the uploads above, the
        # producer of `samples`) must be done first (cf. diagnostics.chain_diagnostics)
        torch.cuda.current_stream(dev).synchronize()
        with ctx.lock:
            return getattr(ctx, device_call)(Ad.data_ptr(), n, k, k, _lib.BMC_ROW_MAJOR,
                                             yd.data_ptr(), t.data_ptr(), C * kept, ld,
                                             *(None if v is None else v.data_ptr() for v in vd),
                                             *tail(A, y, vecs))

    s = np.asarray(samples)
    if s.dtype != np.float64:
        raise ValueError(f"samples must be float64; got {s.dtype}")
    n, k, C, T, kept = _check_shapes(A.shape, y.shape, s.shape, burn, thin, min_points)
    vecs = _point_vectors(vectors, n)
    s = (s if s.ndim == 3 else s[None])[:, burn::thin]
    st = s.strides
    if st[2] == 8 and st[1] % 8 == 0 and st[1] >= 8 * (k + 1) and (C == 1 or st[0] == kept * st[1]):
        ld = st[1] // 8   # one strided run of rows (a column subset, thinned draws): read in place
    else:
        s = np.ascontiguousarray(s)
        ld = k + 1
    A, lda, layout = _host_matrix(A)
    y = np.ascontiguousarray(y)
    ctx = _lib.default_context(device)
    with ctx.lock:
        return getattr(ctx, host_call)(A, n, k, lda, layout, y, s, C * kept, ld, *vecs,
                                       *tail(A, y, vecs))


def _check_nu(nu):
    """None (the Gaussian likelihood) or the Student-t degrees of freedom as a float; ValueError
    for anything not positive and finite (no GPU needed)."""
    if nu is None:
        return None
    if isinstance(nu, bool) or not isinstance(nu, (int, float, np.integer, np.floating)):
        raise ValueError(f"nu must be None or a positive finite number; got {nu!r}")
    nu = float(nu)
    if not (0.0 < nu < float("inf")):
        raise ValueError(f"nu must be None or a positive finite number; got {nu}")
    return nu


MAX_NU_VALUES = 4096


def _nu_table(nu_draws, samples, burn, thin):
    """(distinct values, int32 index per pooled kept draw) of ``nu_draws``, shaped like the leading
    dimensions of ``samples`` and burnt, thinned and pooled like them; ValueError otherwise (no GPU
    needed)."""
    if _is_torch(nu_draws):
        nu_draws = nu_draws.detach().cpu().numpy()
    nd = np.asarray(nu_draws, dtype=np.float64)
    lead = tuple(samples.shape)[:-1]
    if len(lead) not in (1, 2) or nd.shape != lead:
        raise ValueError(f"nu_draws must be shaped like the leading dimensions of samples {lead}; "
                         f"got {nd.shape}")
    burn = _check_int("burn", burn, 0)
    thin = _check_int("thin", thin, 1)
    nd = (nd if nd.ndim == 2 else nd[None])[:, burn::thin].reshape(-1)
    if not (np.all(np.isfinite(nd)) and np.all(nd > 0)):
        raise ValueError("nu_draws must be positive and finite")
    values, index = np.unique(nd, return_inverse=True)
    if values.shape[0] > MAX_NU_VALUES:
        raise ValueError(f"nu_draws holds {values.shape[0]} distinct values; at most {MAX_NU_VALUES}")
    return values, np.ascontiguousarray(index.reshape(-1), dtype=np.int32)


def _likelihood_call(name, nu, nu_draws=None, samples=None, burn=0, thin=1):
    """(host method, device method, trailing scalars, what must stay alive during the call) of a
    scoring call under the likelihood."""
    if nu_draws is not None:
        if nu is not None:
            raise ValueError("give nu (one value for all draws) or nu_draws (one per draw), not both")
        values, index = _nu_table(nu_draws, samples, burn, thin)
        if _is_torch(samples) and samples.is_cuda:
            import torch
            held = torch.as_tensor(index, device=samples.device)
            return name + "_tv", name + "_tv_device", (values, held.data_ptr()), held
        return name + "_tv", name + "_tv_device", (values, index), index
    nu = _check_nu(nu)
    if nu is None:
        return name, name + "_device", (), None
    return name + "_t", name + "_t_device", (nu,), None


def pointwise_log_likelihood(A, y, samples, burn=0, thin=1, device=0, nu=None, nu_draws=None):
    """``lppd_i``, ``p_waic_i`` and ``mean_ll_i`` of every row of ``A`` (module docstring).

    ``A`` is ``(n_points, k)`` float64 (either memory order: ``U_hat`` is Fortran-ordered), ``y``
    ``(n_points,)``.  ``samples`` is ``(T, k+1)`` or ``(C, T, k+1)`` float64, the samplers' layout
    (last column sigma): a numpy array, or a CUDA torch tensor whose last dimension is contiguous
    (read in place; ``device`` is then the tensor's).  The first ``burn`` draws of every chain are
    dropped, every ``thin``-th of the rest kept, and the chains pooled.  Returns a dict of
    ``[n_points]`` arrays ``lppd``, ``p_waic``, ``mean_ll``.  ``nu=None`` is the Gaussian
    likelihood; a positive finite number the Student-t one with that many degrees of freedom.
    ``nu_draws`` (instead of ``nu``) is the Student-t likelihood with a ``nu`` per draw, for a fit
    that estimated it: an array shaped like the leading dimensions of ``samples`` (``(T,)`` or
    ``(C, T)``), burnt, thinned and pooled like them; at most 4096 distinct values."""
    host, dev, scalars, held = _likelihood_call("pointwise_loglik", nu, nu_draws, samples, burn, thin)
    out = _pointwise_call(host, dev, A, y, samples, burn, thin, device, scalars=scalars)
    del held
    return out


def _se(v):
    n = v.shape[0]
    return float(np.sqrt(n * np.var(v, ddof=1))) if n > 1 else float("nan")


def waic_summary(lppd, p_waic):
    """The WAIC summary of the module docstring from the pointwise vectors (host, float64)."""
    lppd = np.asarray(lppd, dtype=np.float64)
    p_waic = np.asarray(p_waic, dtype=np.float64)
    elpd_i = lppd - p_waic
    elpd = float(np.sum(elpd_i))
    return {"elpd_waic": elpd, "p_waic": float(np.sum(p_waic)), "waic": -2.0 * elpd,
            "se": _se(elpd_i), "n_high_p": int(np.sum(p_waic > HIGH_P_WAIC)),
            "n_points": int(lppd.shape[0])}


def elpd_summary(lppd):
    """Held-out log predictive density: ``elpd = sum_i lppd_i`` and its standard error."""
    lppd = np.asarray(lppd, dtype=np.float64)
    return {"elpd": float(np.sum(lppd)), "se": _se(lppd), "n_points": int(lppd.shape[0])}


def waic(A, y, samples, burn=0, thin=1, device=0, nu=None, nu_draws=None):
    """WAIC of a fit on its training data: ``elpd_waic``, ``p_waic``, ``waic``, ``se``,
    ``n_high_p``, ``n_points`` and the pointwise ``lppd``, ``p_waic_i``, ``mean_ll``,
    ``elpd_waic_i``.  Arguments as ``pointwise_log_likelihood``."""
    pw = pointwise_log_likelihood(A, y, samples, burn=burn, thin=thin, device=device, nu=nu,
                                  nu_draws=nu_draws)
    out = waic_summary(pw["lppd"], pw["p_waic"])
    out.update(lppd=pw["lppd"], p_waic_i=pw["p_waic"], mean_ll=pw["mean_ll"],
               elpd_waic_i=pw["lppd"] - pw["p_waic"])
    return out


def loo_summary(elpd_loo_i, lppd, pareto_k, n_draws):
    """The PSIS-LOO summary of the module docstring from the pointwise vectors (host, float64);
    ``n_draws`` is the number of pooled kept draws S (for ``k_threshold``)."""
    e = np.asarray(elpd_loo_i, dtype=np.float64)
    lppd = np.asarray(lppd, dtype=np.float64)
    kh = np.asarray(pareto_k, dtype=np.float64)
    elpd = float(np.sum(e))
    thr = min(1.0 - 1.0 / np.log10(n_draws), HIGH_PARETO_K)
    return {"elpd_loo": elpd, "p_loo": float(np.sum(lppd - e)), "looic": -2.0 * elpd, "se": _se(e),
            "n_high_k": int(np.sum(kh > HIGH_PARETO_K)), "k_threshold": float(thr),
            "n_above_threshold": int(np.sum(kh > thr)), "n_points": int(e.shape[0]),
            "n_draws": int(n_draws)}


def psis_loo(A, y, samples, burn=0, thin=1, device=0, nu=None, nu_draws=None):
    """PSIS-LOO of a fit on its training data (module docstring): ``elpd_loo``, ``p_loo``,
    ``looic``, ``se``, ``n_high_k``, ``k_threshold``, ``n_above_threshold``, ``n_points``,
    ``n_draws`` and the pointwise ``elpd_loo_i``, ``p_loo_i``, ``pareto_k``, ``lppd``.  Arguments
    as ``pointwise_log_likelihood``, ``nu`` and ``nu_draws`` included.  The relative efficiency r_eff of the draws is taken as 1, as
    ``loo::psis`` does when none is given.  ``pareto_k`` is ``+inf`` where nothing was smoothed
    (fewer than 25 draws, a tail of equal values, a non-finite fit)."""
    host, dev, scalars, held = _likelihood_call("psis_loo", nu, nu_draws, samples, burn, thin)
    pw = _pointwise_call(host, dev, A, y, samples, burn, thin, device, scalars=scalars)
    del held
    sh = tuple(samples.shape)
    C, T = (1, sh[0]) if len(sh) == 2 else sh[:2]
    out = loo_summary(pw["elpd_loo"], pw["lppd"], pw["pareto_k"], C * kept_draws(T, burn, thin))
    out.update(elpd_loo_i=pw["elpd_loo"], p_loo_i=pw["lppd"] - pw["elpd_loo"],
               pareto_k=pw["pareto_k"], lppd=pw["lppd"])
    return out


PIT_LEVELS = tuple(range(0, 101, 5))


def loo_predict_summary(y, loo_mean, loo_pit, ess):
    """``loo_rmse``, ``pit_coverage`` (21 percentages, levels ``PIT_LEVELS``) and ``min_ess`` of
    the module docstring from the pointwise vectors (host, float64)."""
    y = np.asarray(y, dtype=np.float64)
    m = np.asarray(loo_mean, dtype=np.float64)
    dev = np.abs(2.0 * np.asarray(loo_pit, dtype=np.float64) - 1.0)
    n = y.shape[0]
    cov = [float(np.count_nonzero(dev <= p / 100.0)) / n * 100.0 for p in PIT_LEVELS]
    return {"loo_rmse": float(np.sqrt(np.mean((y - m) ** 2))), "pit_coverage": cov,
            "min_ess": float(np.min(np.asarray(ess, dtype=np.float64)))}


LOO_PREDICT_NU_RANGE = (0.06, 1000.0)


def _check_predict_nu(values):
    """The degrees of freedom the leave-one-out predictive distribution takes: the range over which
    the device's t distribution function is held to its accuracy bar (no GPU needed)."""
    lo, hi = LOO_PREDICT_NU_RANGE
    v = np.asarray(values, dtype=np.float64)
    if not np.all((v >= lo) & (v <= hi)):
        raise ValueError(f"psis_loo_predict takes degrees of freedom between {lo} and {hi:g}; got "
                         f"{float(v.min()):g} .. {float(v.max()):g}")


def psis_loo_predict(A, y, samples, burn=0, thin=1, device=0, nu=None, nu_draws=None):
    """PSIS-LOO with the leave-one-out predictive distribution of every training point (module
    docstring): everything ``psis_loo`` returns, the pointwise ``loo_mean``, ``loo_sd``,
    ``loo_pit``, ``ess`` and ``loo_rmse``, ``pit_coverage``, ``min_ess``.  Arguments as
    ``pointwise_log_likelihood``, ``nu`` and ``nu_draws`` included; ``loo_mean`` is in the space of
    ``A`` and ``y``.  Under the Student-t likelihood ``loo_mean`` is the location of the predictive
    distribution (its mean where ``nu > 1``), ``loo_sd`` is ``+inf`` at every point that is not NaN
    when a scored ``nu`` is at most 2, and every ``nu`` must lie in 0.06 .. 1000 (``ValueError``)."""
    host, dev, scalars, held = _likelihood_call("psis_loo_predict", nu, nu_draws, samples, burn, thin)
    if scalars:
        _check_predict_nu(scalars[0])
    pw = _pointwise_call(host, dev, A, y, samples, burn, thin, device, scalars=scalars)
    del held
    sh = tuple(samples.shape)
    C, T = (1, sh[0]) if len(sh) == 2 else sh[:2]
    out = loo_summary(pw["elpd_loo"], pw["lppd"], pw["pareto_k"], C * kept_draws(T, burn, thin))
    out.update(elpd_loo_i=pw["elpd_loo"], p_loo_i=pw["lppd"] - pw["elpd_loo"],
               pareto_k=pw["pareto_k"], lppd=pw["lppd"], loo_mean=pw["loo_mean"],
               loo_sd=pw["loo_sd"], loo_pit=pw["loo_pit"], ess=pw["ess"])
    out.update(loo_predict_summary(np.asarray(y), pw["loo_mean"], pw["loo_pit"], pw["ess"]))
    return out


ELPD_KINDS = (("elpd_loo_i", "elpd_loo"), ("elpd_waic_i", "elpd_waic"), ("elpd_cv_i", "elpd_cv"),
              ("lppd", "elpd"))


def compare_elpd(fits):
    """Compare fits of the same data by their expected log predictive density (host, float64).

    ``fits`` maps a name to a result dict of ``psis_loo``, ``waic``, ``kfold_cv`` or
    ``log_predictive_density`` (``BayesianModelCombination.score`` returns the first, second or
    last); the pointwise vector is ``elpd_loo_i``, ``elpd_waic_i``, ``elpd_cv_i`` or ``lppd``.
    Every entry must be of the same kind and the same length, else ``ValueError``.  Returns a dict:
    ``names`` ordered by ``elpd`` descending (ties in input order), ``elpd`` and ``se`` in that
    order, ``elpd_diff[j] = elpd[best] - elpd[j]``, ``se_diff[j] = sqrt(n var_i(e_best,i - e_j,i,
    ddof=1))`` (0 at the best: the paired standard error, as ``cv.path_summary``), ``kind`` (the
    name of the pointwise vector) and ``n_points``.  NaNs propagate."""
    if not isinstance(fits, dict) or not fits:
        raise ValueError("fits must be a non-empty dict of name -> result dict")
    kind, vectors = None, []
    for name, res in fits.items():
        found = None
        if isinstance(res, dict):
            # (a psis_loo or waic result carries lppd too: the first match names the kind)
            found = next((key for key, total in ELPD_KINDS if key in res and total in res), None)
        if found is None:
            raise ValueError(f"fits[{name!r}] is not a result of psis_loo, waic, kfold_cv or "
                             "log_predictive_density")
        if kind is not None and found != kind:
            raise ValueError(f"fits[{name!r}] holds {found}, the entries before it {kind}: "
                             "only scores of the same kind compare")
        kind = found
        v = np.asarray(res[found], dtype=np.float64)
        if v.ndim != 1 or (vectors and v.shape != vectors[0].shape):
            raise ValueError(f"fits[{name!r}][{found!r}] must be a vector of the length of the "
                             "other entries (the same data points)")
        vectors.append(v)
    e = np.stack(vectors)                                   # (fits, n)
    n = e.shape[1]
    elpd = e.sum(axis=1)
    # descending, ties in input order; a NaN elpd sorts last
    order = sorted(range(len(vectors)), key=lambda j: (np.isnan(elpd[j]), -elpd[j]))
    e, elpd = e[order], elpd[order]
    d = e[0][None, :] - e
    with np.errstate(invalid="ignore"):
        se = np.sqrt(n * np.var(e, axis=1, ddof=1)) if n > 1 else np.full(len(order), np.nan)
        se_diff = np.sqrt(n * np.var(d, axis=1, ddof=1)) if n > 1 else np.full(len(order), np.nan)
    se_diff[0] = 0.0
    names = list(fits)
    return {"names": [names[j] for j in order], "elpd": elpd, "se": se, "elpd_diff": elpd[0] - elpd,
            "se_diff": se_diff, "kind": kind, "n_points": int(n)}
