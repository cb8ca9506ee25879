"""Dense numpy reference of the Student-t scores of pybmc_amd.scoring (``nu=`` of
``pointwise_log_likelihood``, ``waic`` and ``psis_loo``): the marginal t density of that module's
docstring under every draw, then the estimators of score_reference / psis_reference unchanged.
Everything in ``dtype`` (float64, or np.longdouble for the rounding floor).  TEST INFRASTRUCTURE
ONLY; shared by test_tscore_host.py and test_tscore_gpu.py."""
import functools
import math

import numpy as np

import psis_reference as PR
import score_reference as R


PI_L = np.longdouble("3.14159265358979323846264338327950288")
# B_2j / (2j (2j - 1)), j = 1 .. 8: Stirling's series of log Gamma
STIRLING = ((1, 12), (-1, 360), (1, 1260), (-1, 1680), (1, 1188), (-691, 360360), (1, 156),
            (-3617, 122400))


def _lgamma(x):
    """log Gamma(x), x > 0, in long double: the recurrence up to x >= 20, then Stirling's series
    (its next term is below 1e-22 there)."""
    x = np.longdouble(x)
    shift = np.longdouble(0)
    while x < 20:
        shift += np.log(x)
        x = x + 1
    series, xi = np.longdouble(0), 1 / x
    for a, b in STIRLING:
        series += np.longdouble(a) / np.longdouble(b) * xi
        xi = xi / (x * x)
    return (x - np.longdouble(0.5)) * np.log(x) - x + np.longdouble(0.5) * np.log(2 * PI_L) + series - shift


def t_constant(nu, dtype=np.float64):
    """lgamma((nu + 1) / 2) - lgamma(nu / 2) - 1/2 log(nu pi): in long double whatever ``dtype`` is
    (the difference of the two lgamma loses digits as nu grows), then rounded to it."""
    nu = np.longdouble(nu)
    return dtype(_lgamma((nu + 1) / 2) - _lgamma(nu / 2) - np.longdouble(0.5) * np.log(nu * PI_L))


def loglik_t(A, y, theta, nu, dtype=np.float64):
    """ll_t[i, s], dense, in ``dtype``."""
    A = np.asarray(A).astype(dtype)
    y = np.asarray(y).astype(dtype)
    theta = np.asarray(theta).astype(dtype)
    nu = dtype(nu)
    sg = theta[:, -1]
    r = y[:, None] - A @ theta[:, :-1].T
    return (t_constant(nu, dtype) - np.log(sg)[None, :]
            - (nu + 1) / 2 * np.log1p(r * r / (nu * sg * sg)[None, :]))


def pointwise(A, y, theta, nu, dtype=np.float64, chunk=256):
    """dict of [n] arrays lppd, p_waic, mean_ll (as score_reference.pointwise)."""
    A = np.asarray(A)
    y = np.asarray(y)
    n, S = A.shape[0], np.asarray(theta).shape[0]
    out = {k: np.empty(n, dtype=dtype) for k in ("lppd", "p_waic", "mean_ll")}
    for i0 in range(0, n, chunk):
        sl = slice(i0, min(n, i0 + chunk))
        with np.errstate(all="ignore"):
            ll = loglik_t(A[sl], y[sl], theta, nu, dtype)
            out["lppd"][sl] = R._lse(ll, 1) - np.log(dtype(S))
            out["p_waic"][sl] = ll.var(axis=1, ddof=1)
            out["mean_ll"][sl] = ll.mean(axis=1)
    return out


def loo_pointwise(A, y, theta, nu, dtype=np.float64, chunk=64):
    """dict of [n] arrays elpd_loo, pareto_k, lppd, p_loo (as psis_reference.pointwise)."""
    A = np.asarray(A)
    y = np.asarray(y)
    n, S = A.shape[0], np.asarray(theta).shape[0]
    out = {key: np.empty(n, dtype=dtype) for key in ("elpd_loo", "pareto_k", "lppd")}
    for i0 in range(0, n, chunk):
        sl = slice(i0, min(n, i0 + chunk))
        with np.errstate(all="ignore"):
            ll = loglik_t(A[sl], y[sl], theta, nu, dtype)
            out["lppd"][sl] = R._lse(ll, 1) - np.log(dtype(S))
        for r in range(ll.shape[0]):
            if not np.isfinite(ll[r]).all():
                out["elpd_loo"][i0 + r] = out["pareto_k"][i0 + r] = np.nan
                continue
            out["elpd_loo"][i0 + r], out["pareto_k"][i0 + r] = PR.psis_row(ll[r], dtype)
    out["p_loo"] = out["lppd"] - out["elpd_loo"]
    return out


# ---- the cases of test_tscore_gpu.py (seeded; no GPU) ------------------------------------------------
NUS = (1.5, 4.0, 50.0)
# (k, n, S): every k meets every S and every n once or more; S = 4097 once
SHAPES = tuple((k, n, S) for k, n in ((1, 1), (4, 63), (5, 65), (17, 130), (33, 65))
               for S in (2, 24, 25, 63, 65, 513)) + ((4, 130, 4097),)


def shape_case(k, n, S):
    return R.random_case(n, k, S, 7000 * k + 10 * n + S)


def outlier_case():
    """A large argument of log1p: target 0 moved 40 units out (r^2 / (nu sigma^2) up to 4000)."""
    A, y, th = R.random_case(65, 5, 513, 4242)
    y = y.copy()
    y[0] += 40.0
    return A, y, th


def tiny_case():
    """Tiny arguments of log1p: every draw's coefficients are exactly 0, so the residual of point i
    is y_i itself, 10^-20 .. 10^-1, with sigma in [0.9, 1.1]: r^2 / (nu sigma^2) from 1e-41 up."""
    n, k, S = 65, 3, 65
    rng = np.random.default_rng(99)
    A = rng.standard_normal((n, k))
    y = 10.0 ** np.linspace(-20, -1, n)
    sig = rng.permutation(np.linspace(0.9, 1.1, S))
    return A, y, np.column_stack([np.zeros((S, k)), sig])


@functools.lru_cache(maxsize=None)
def reference(kind, key, nu):
    """The float64 reference of a case, computed once: (pointwise, loo_pointwise)."""
    A, y, th = case_arrays(kind, key)
    return pointwise(A, y, th, nu), loo_pointwise(A, y, th, nu)


# ---- bars: 100 x the float64 floor of this reference against long double on random_case shapes ---
BAR_LPPD = 1e-11      # |d lppd_i| / max(1, |ref|)        (the bar of test_scoring_gpu.py)
BAR_REL = 1e-11       # p_waic_i and mean_ll_i, relative  (the bar of test_scoring_gpu.py)
BAR_ELPD = 2.1e-13    # |d elpd_loo_i| / max(1, |ref|)    (floor 2.1e-15)
BAR_K = 3.4e-12       # |d pareto_k|, where finite        (floor 3.4e-14)


def all_cases():
    """(tag, kind, key) of every case the GPU file checks against this reference."""
    for shape in SHAPES:
        yield "k=%d n=%d S=%d" % shape, "shape", shape
    yield "outlier", "outlier", None
    yield "tiny", "tiny", None


def case_arrays(kind, key):
    return {"shape": lambda: shape_case(*key), "outlier": outlier_case, "tiny": tiny_case}[kind]()


def deviations(got, ref_pw, ref_loo):
    """Worst deviations of (pointwise, loo) results from a reference, in the units of the bars:
    dict lppd, p_waic, mean_ll, elpd_loo, pareto_k; pareto_k must be infinite where the reference's
    is (KeyError-free: pass None for a part that was not computed)."""
    out = {}
    f = lambda v: np.asarray(v, dtype=np.longdouble)
    if got[0] is not None:
        g, r = got[0], ref_pw
        out["lppd"] = float(np.max(np.abs(f(g["lppd"]) - f(r["lppd"])) / np.maximum(1, np.abs(f(r["lppd"])))))
        for key in ("p_waic", "mean_ll"):
            out[key] = float(np.max(np.abs(f(g[key]) - f(r[key])) / (np.abs(f(r[key])) + 1e-24 / BAR_REL)))
    if got[1] is not None:
        g, r = got[1], ref_loo
        out["loo_lppd"] = float(np.max(np.abs(f(g["lppd"]) - f(r["lppd"])) / np.maximum(1, np.abs(f(r["lppd"])))))
        out["elpd_loo"] = float(np.max(np.abs(f(g["elpd_loo"]) - f(r["elpd_loo"]))
                                       / np.maximum(1, np.abs(f(r["elpd_loo"])))))
        gk, rk = np.asarray(g["pareto_k"], dtype=np.float64), np.asarray(r["pareto_k"], dtype=np.float64)
        assert np.array_equal(np.isinf(gk), np.isinf(rk)) and not np.isnan(gk).any()
        fin = np.isfinite(rk)
        out["pareto_k"] = float(np.max(np.abs(f(g["pareto_k"])[fin] - f(r["pareto_k"])[fin]))) if fin.any() else 0.0
    return out
