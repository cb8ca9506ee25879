"""Dense numpy reference of pybmc_amd.scoring (the estimator of that module's docstring):
pointwise log-likelihood of the Gaussian model under every draw, log-mean-exp, variance (ddof 1)
and mean over the draws, and the WAIC / held-out summaries.  Chunked over points when large."""
import numpy as np
from scipy.special import logsumexp

HIGH_P_WAIC = 0.4


def loglik(A, y, theta, dtype=np.float64):
    """ll[i, s], dense, in ``dtype`` (np.longdouble for the rounding-floor check)."""
    A = np.asarray(A).astype(dtype)
    y = np.asarray(y).astype(dtype)
    theta = np.asarray(theta).astype(dtype)
    sg = theta[:, -1]
    r = y[:, None] - A @ theta[:, :-1].T
    return (-dtype(0.5) * np.log(2 * dtype(np.pi)) - np.log(sg)[None, :]
            - r * r / (2 * sg * sg)[None, :])


def _lse(ll, axis):
    if ll.dtype == np.float64:
        return logsumexp(ll, axis=axis)
    m = ll.max(axis=axis, keepdims=True)   # (scipy's logsumexp would fall back to float64)
    return np.squeeze(m, axis) + np.log(np.exp(ll - m).sum(axis=axis))


def pointwise(A, y, theta, dtype=np.float64, chunk=256):
    """dict of [n] arrays lppd, p_waic, mean_ll."""
    A = np.asarray(A)
    y = np.asarray(y)
    n, S = A.shape[0], np.asarray(theta).shape[0]
    out = {k: np.empty(n, dtype=dtype) for k in ("lppd", "p_waic", "mean_ll")}
    for i0 in range(0, n, chunk):
        sl = slice(i0, min(n, i0 + chunk))
        with np.errstate(all="ignore"):
            ll = loglik(A[sl], y[sl], theta, dtype)
            out["lppd"][sl] = _lse(ll, 1) - np.log(dtype(S))
            out["p_waic"][sl] = ll.var(axis=1, ddof=1)
            out["mean_ll"][sl] = ll.mean(axis=1)
    return out


def pointwise_online(A, y, theta, blk=64):
    """The same in the order a tiled kernel works: per 64-draw tile a running max with one rescale
    and a (mean, centred M2) pair merged by Chan's formula.  float64."""
    A, y, theta = (np.asarray(v, dtype=np.float64) for v in (A, y, theta))
    n, S = len(y), len(theta)
    M = np.full(n, -np.inf)
    L = np.zeros(n)
    cnt, mean, M2 = 0, np.zeros(n), np.zeros(n)
    for s0 in range(0, S, blk):
        ll = loglik(A, y, theta[s0:s0 + blk])
        m = np.maximum(M, ll.max(1))
        L = L * np.exp(M - m) + np.exp(ll - m[:, None]).sum(1)
        M = m
        b = ll.shape[1]
        mb = ll.mean(1)
        m2b = ((ll - mb[:, None]) ** 2).sum(1)
        d = mb - mean
        tot = cnt + b
        mean = mean + d * b / tot
        M2 = M2 + m2b + d * d * cnt * b / tot
        cnt = tot
    return {"lppd": M + np.log(L) - np.log(S), "p_waic": M2 / (cnt - 1), "mean_ll": mean}


def _se(v):
    n = len(v)
    return float(np.sqrt(n * np.var(v, ddof=1))) if n > 1 else float("nan")


def waic_summary(pw):
    e = np.asarray(pw["lppd"], dtype=np.float64) - np.asarray(pw["p_waic"], dtype=np.float64)
    return {"elpd_waic": float(e.sum()), "p_waic": float(np.sum(pw["p_waic"])),
            "waic": -2.0 * float(e.sum()), "se": _se(e),
            "n_high_p": int(np.sum(np.asarray(pw["p_waic"]) > HIGH_P_WAIC)), "n_points": len(e)}


def elpd_summary(pw):
    l = np.asarray(pw["lppd"], dtype=np.float64)
    return {"elpd": float(l.sum()), "se": _se(l), "n_points": len(l)}


def pool(samples, burn=0, thin=1):
    """(C, T, k+1) or (T, k+1) -> the kept draws of every chain, concatenated."""
    s = np.asarray(samples)
    s = s if s.ndim == 3 else s[None]
    return np.concatenate([c[burn::thin] for c in s], axis=0)


# ---- the synthetic cases of the tests (seeded; no GPU) -------------------------------------------
CASES = {   # name: (n_points, n_models, components kept, draws, noise)
    "c1": (377, 4, 3, 20000, 0.5),
    "c2ish": (1500, 33, 32, 12000, 0.1),
    "tight": (1500, 9, 8, 12000, 1e-3),
}


def synth_case(name, outlier=True):
    """(A, y, theta): orthonormal design of a centred random frame, a target with Gaussian noise,
    draws scattered about the least-squares point like a posterior (sd = noise per coefficient,
    sigma within 1/sqrt(2n) of the noise); target 0 moved 40 sigma out (lppd_0 about -700)."""
    n, km, kept, S, noise = CASES[name]
    rng = np.random.default_rng(1)
    F = rng.standard_normal((n, km))
    U = np.linalg.svd(F - F.mean(1, keepdims=True), full_matrices=False)[0]
    A = np.ascontiguousarray(U[:, :kept])
    y = A @ rng.standard_normal(kept) + noise * rng.standard_normal(n)
    rng = np.random.default_rng(2)
    sig = noise * (1 + rng.standard_normal(S) / np.sqrt(2 * n))
    beta = A.T @ y + sig[:, None] * rng.standard_normal((S, kept))
    if outlier:
        y = y.copy()
        y[0] += 40 * noise
    return A, y, np.column_stack([beta, sig])


def three_component_frame(n, seed, n_models=6, noise=0.1):
    """A model frame whose errors have THREE common components of clearly different size: model m
    predicts truth + sum_c L[c, m] z_c + small private noise, with loadings whose mean over the
    models is not zero, so the centred truth depends on all three z_c.  Keeping one component
    leaves the other two in the residual (sd about 1 against the 0.1 noise)."""
    import pandas as pd
    rng = np.random.default_rng(seed)
    lrng = np.random.default_rng(12345)          # the loadings belong to the models, not the split
    L = lrng.standard_normal((3, n_models)) * np.array([4.0, 2.0, 1.0])[:, None]
    L += np.array([1.5, -1.0, 0.8])[:, None]     # non-zero mean over the models
    z = rng.standard_normal((n, 3))
    truth0 = 10.0 + 3.0 * rng.standard_normal(n)
    F = truth0[:, None] + z @ L + 0.02 * rng.standard_normal((n, n_models))
    models = [f"m{i}" for i in range(n_models)]
    df = pd.DataFrame(F, columns=models)
    df["truth"] = truth0 + noise * rng.standard_normal(n)
    df["idx"] = np.arange(n)
    return df, models


def random_case(n, k, S, seed):
    """(A, y, theta) of any shape on which the reference itself is well conditioned: var_s ll
    loses digits where the ll[i, .] of a point nearly coincide (two draws: relative error
    eps |ll| / |ll_1 - ll_2|), so the sigmas are spread evenly over [0.5, 1.5] and the residuals
    kept below the smallest of them (two Gaussians of widths a < b cross at r^2 > a^2 = 0.25: no
    point sits on a crossing).  test_scoring_host.py holds the float64 reference on these cases to
    1e-13 of extended precision, 1/100 of the device bound."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, k)) / np.sqrt(k)
    b = rng.standard_normal(k)
    y = A @ b + 0.25 * (2 * rng.random(n) - 1)
    sig = rng.permutation(np.linspace(0.5, 1.5, S))
    th = np.column_stack([b + 0.03 * rng.standard_normal((S, k)), sig])
    return A, y, th


SHAPE_K = (1, 3, 4, 5, 31, 32, 33, 256)
SHAPE_N = (1, 63, 64, 65, 1000)
SHAPE_S = (2, 63, 64, 65, 4097)


def shape_cases(k):
    """The 25 (n, S) cases of one k, seeded as the GPU test seeds them."""
    case = 0
    for n in SHAPE_N:
        for S in SHAPE_S:
            yield case, n, S, random_case(n, k, S, 1000 * k + case)
            case += 1
