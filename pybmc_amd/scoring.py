"""Scoring a sampled fit on the GPU: pointwise log predictive density and WAIC.

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

S. Watanabe, "Asymptotic equivalence of Bayes cross validation and widely applicable information
criterion in singular learning theory", JMLR 11, 2010; A. Gelman, J. Hwang, A. Vehtari,
"Understanding predictive information criteria for Bayesian models", Stat. Comput. 24, 2014.

On the device (``kernels_waic.hip``) the n x S matrix is never stored: an f64 MFMA GEMM whose
tiles are reduced in the epilogue.  Non-finite input gives NaN outputs, not an error.
"""
from __future__ import annotations

import numpy as np

POINTWISE_KEYS = ("lppd", "p_waic", "mean_ll")
HIGH_P_WAIC = 0.4
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


def _check_shapes(a_shape, y_shape, s_shape, burn, thin):
    """(n, k, C, T, kept per chain) of valid arguments; ValueError otherwise (no GPU needed)."""
    burn = _check_int("burn", burn, 0)
    thin = _check_int("thin", thin, 1)
    if len(a_shape) != 2:
        raise ValueError(f"A must be (n_points, k); got {len(a_shape)} dimensions")
    n, k = a_shape
    if n < 1:
        raise ValueError("A must hold at least one point")
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


def pointwise_log_likelihood(A, y, samples, burn=0, thin=1, device=0):
    """``lppd_i``, ``p_waic_i`` and ``mean_ll_i`` of every row of ``A`` (module docstring).

    ``A`` is ``(n_points, k)`` float64 (either memory order: ``U_hat`` is Fortran-ordered), ``y``
    ``(n_points,)``.  ``samples`` is ``(T, k+1)`` or ``(C, T, k+1)`` float64, the samplers' layout
    (last column sigma): a numpy array, or a CUDA torch tensor whose last dimension is contiguous
    (read in place; ``device`` is then the tensor's).  The first ``burn`` draws of every chain are
    dropped, every ``thin``-th of the rest kept, and the chains pooled.  Returns a dict of
    ``[n_points]`` arrays ``lppd``, ``p_waic``, ``mean_ll``."""
    from . import _lib

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
        n, k, C, T, kept = _check_shapes(A.shape, y.shape, tuple(samples.shape), burn, thin)
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
        # the library reads on its own stream: what torch queued (the uploads above, the
        # producer of `samples`) must be done first (cf. diagnostics.chain_diagnostics)
        torch.cuda.current_stream(dev).synchronize()
        with ctx.lock:
            return ctx.pointwise_loglik_device(Ad.data_ptr(), n, k, k, _lib.BMC_ROW_MAJOR,
                                               yd.data_ptr(), t.data_ptr(), C * kept, ld)

    s = np.asarray(samples)
    if s.dtype != np.float64:
        raise ValueError(f"samples must be float64; got {s.dtype}")
    n, k, C, T, kept = _check_shapes(A.shape, y.shape, s.shape, burn, thin)
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
        return ctx.pointwise_loglik(A, n, k, lda, layout, y, s, C * kept, ld)


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


def waic(A, y, samples, burn=0, thin=1, device=0):
    """WAIC of a fit on its training data: ``elpd_waic``, ``p_waic``, ``waic``, ``se``,
    ``n_high_p``, ``n_points`` and the pointwise ``lppd``, ``p_waic_i``, ``mean_ll``,
    ``elpd_waic_i``.  Arguments as ``pointwise_log_likelihood``."""
    pw = pointwise_log_likelihood(A, y, samples, burn=burn, thin=thin, device=device)
    out = waic_summary(pw["lppd"], pw["p_waic"])
    out.update(lppd=pw["lppd"], p_waic_i=pw["p_waic"], mean_ll=pw["mean_ll"],
               elpd_waic_i=pw["lppd"] - pw["p_waic"])
    return out
