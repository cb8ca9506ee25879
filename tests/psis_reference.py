"""Dense numpy restatement of PSIS-LOO (Vehtari, Gelman & Gabry 2017; Vehtari, Simpson, Gelman,
Yao & Gabry 2024; the generalised Pareto fit of Zhang & Stephens 2009 as loo::gpdfit does it),
written from the papers and the estimator's definition, not from pybmc_amd.scoring.  Everything in
``dtype`` (float64, or np.longdouble for the rounding floor).  r_eff = 1.

Per point, over the S draws: lw = -ll, shifted to a largest of 0; M = min(S // 5, ceil(3 sqrt S));
the M largest lw are the tail, the next one the cutoff; a generalised Pareto fit of
exp(tail) - exp(cutoff); the tail replaced in rank order by the fit's quantiles; truncation at 0;
elpd_loo_i = logsumexp(ll + lw) - logsumexp(lw)."""
import math

import numpy as np

import score_reference as R

HIGH_K = 0.7
MIN_TAIL = 5


def tail_length(S):
    return min(S // 5, int(math.ceil(3.0 * math.sqrt(S))))


def gpdfit(x, dtype=np.float64):
    """(k, sigma) of ascending positive x; k with the weak prior (M k + 5) / (M + 10)."""
    x = np.asarray(x, dtype=dtype)
    M = len(x)
    m = 30 + int(math.floor(math.sqrt(M)))
    prior = dtype(3)
    xq = x[int(math.floor(M / 4 + 0.5)) - 1]
    j = np.arange(1, m + 1).astype(dtype)
    with np.errstate(all="ignore"):
        theta = 1 / x[-1] + (1 - np.sqrt(dtype(m) / (j - dtype(0.5)))) / (prior * xq)
        kj = np.log1p(-theta[:, None] * x[None, :]).mean(axis=1)
        lj = M * (np.log(-theta / kj) - kj - 1)
        w = 1 / np.exp(lj[None, :] - lj[:, None]).sum(axis=1)    # w_j = 1 / sum_i exp(l_i - l_j)
        th = (w * theta).sum()
        k = np.log1p(-th * x).mean()
        sigma = -k / th
        k = (M * k + 5) / (M + 10)
    return k, sigma


def undo_prior(k, M):
    return (k * (M + 10) - 5) / M


def psis_row(ll, dtype=np.float64):
    """(elpd_loo_i, pareto_k) of one point's ll[s]."""
    ll = np.asarray(ll, dtype=dtype)
    S = len(ll)
    lw = -ll
    lw = lw - lw.max()
    M = tail_length(S)
    khat = dtype(np.inf)
    if M >= MIN_TAIL:
        order = np.argsort(lw, kind="stable")
        tail = order[S - M:]                  # ascending lw
        cutoff = lw[order[S - M - 1]]
        lt = lw[tail]
        if lt[0] != lt[-1]:
            with np.errstate(all="ignore"):
                ecut = np.exp(cutoff)
                k, sigma = gpdfit(np.exp(lt) - ecut, dtype)
                if np.isfinite(k):
                    khat = k
                    p = (np.arange(1, M + 1).astype(dtype) - dtype(0.5)) / M
                    if abs(k) < 1e-30:
                        q = -sigma * np.log1p(-p)
                    else:
                        q = sigma * np.expm1(-k * np.log1p(-p)) / k
                    lw = lw.copy()
                    lw[tail] = np.log(ecut + q)
        lw = np.minimum(lw, 0)
    with np.errstate(all="ignore"):
        a = ll + lw
        num = a.max() + np.log(np.exp(a - a.max()).sum())
        den = lw.max() + np.log(np.exp(lw - lw.max()).sum())
    return num - den, khat


def pointwise(A, y, theta, dtype=np.float64, chunk=64):
    """dict of [n] arrays elpd_loo, pareto_k, lppd, p_loo (non-finite ll of a point: NaN)."""
    A = np.asarray(A)
    y = np.asarray(y)
    n, S = A.shape[0], np.asarray(theta).shape[0]
    out = {key: np.empty(n, dtype=dtype) for key in ("elpd_loo", "pareto_k", "lppd")}
    for i0 in range(0, n, chunk):
        sl = slice(i0, min(n, i0 + chunk))
        with np.errstate(all="ignore"):
            ll = R.loglik(A[sl], y[sl], theta, dtype)
            out["lppd"][sl] = R._lse(ll, 1) - np.log(dtype(S))
        for r in range(ll.shape[0]):
            if not np.isfinite(ll[r]).all():
                out["elpd_loo"][i0 + r] = out["pareto_k"][i0 + r] = np.nan
                continue
            out["elpd_loo"][i0 + r], out["pareto_k"][i0 + r] = psis_row(ll[r], dtype)
    out["p_loo"] = out["lppd"] - out["elpd_loo"]
    return out


def _se(v):
    n = len(v)
    return float(np.sqrt(n * np.var(v, ddof=1))) if n > 1 else float("nan")


def loo_summary(pw, S):
    e = np.asarray(pw["elpd_loo"], dtype=np.float64)
    k = np.asarray(pw["pareto_k"], dtype=np.float64)
    thr = min(1.0 - 1.0 / math.log10(S), HIGH_K)
    return {"elpd_loo": float(e.sum()),
            "p_loo": float(np.sum(np.asarray(pw["lppd"], dtype=np.float64) - e)),
            "looic": -2.0 * float(e.sum()), "se": _se(e), "n_high_k": int(np.sum(k > HIGH_K)),
            "k_threshold": thr, "n_above_threshold": int(np.sum(k > thr)), "n_points": len(e),
            "n_draws": int(S)}


# ---- cases ------------------------------------------------------------------------------------------
GOLDEN = ("gibbs_ortho629x3", "gibbs_dense64x8", "gibbs_ragged1237x5", "simplex_synth150x4")

SHAPE_N = (1, 63, 64, 65, 1000)
SHAPE_S = (2, 24, 25, 63, 64, 65, 4097)


def shape_cases(k):
    """The 35 (n, S) cases of one k, seeded as the GPU test seeds them (R.random_case inputs)."""
    case = 0
    for n in SHAPE_N:
        for S in SHAPE_S:
            yield case, n, S, R.random_case(n, k, S, 5000 * k + case)
            case += 1


def closed_form_case(n, k, S, seed, sigma=0.7, leverage=0.5):
    """Orthonormal A whose row 0 carries h_0 of about ``leverage``, fixed sigma, beta_s ~ N(A'y, sigma^2 I):
    the exact leave-one-out predictive density of point i is
    N(y_i; y_i - r_i / (1 - h_i), sigma^2 / (1 - h_i)), h_i = |a_i|^2, r_i the full-fit residual.
    Returns (A, y, theta, exact elpd_loo_i, exact in-sample lpd_i)."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, k))
    G[0, 0] = 0.0
    G[:, 0] *= np.sqrt((1 - leverage) / np.sum(G[:, 0] ** 2))
    G[0, 0] = np.sqrt(leverage)          # a unit first column with leverage in row 0
    G[0, 1:] = 0.0                       # (the other columns add O(1/n) to h_0)
    A = np.ascontiguousarray(np.linalg.qr(G)[0])
    y = A @ rng.standard_normal(k) + sigma * rng.standard_normal(n)
    bhat = A.T @ y
    theta = np.column_stack([bhat + sigma * rng.standard_normal((S, k)), np.full(S, sigma)])
    h = np.sum(A * A, axis=1)
    r = y - A @ bhat
    v = sigma ** 2 / (1 - h)
    exact = -0.5 * np.log(2 * np.pi * v) - (r / (1 - h)) ** 2 / (2 * v)
    v_in = sigma ** 2 * (1 + h)
    lpd = -0.5 * np.log(2 * np.pi * v_in) - r ** 2 / (2 * v_in)
    return A, y, theta, exact, lpd
