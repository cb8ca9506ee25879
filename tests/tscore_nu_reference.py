"""Dense numpy reference of the Student-t scores with a nu per draw (``nu_draws=`` of
``pointwise_log_likelihood``, ``waic`` and ``psis_loo``): the density of tscore_reference.loglik_t
with draw s's own nu_s, then the estimators of score_reference / psis_reference unchanged.  Everything
in ``dtype`` (float64, or np.longdouble for the rounding floor).  TEST INFRASTRUCTURE ONLY; shared by
test_tscore_nu_host.py and test_tscore_nu_gpu.py."""
import functools

import numpy as np

import psis_reference as PR
import score_reference as R
import tscore_reference as T


def loglik_tv(A, y, theta, nu_draws, dtype=np.float64):
    """ll[i, s] under t_{nu_s}, dense, in ``dtype``."""
    A = np.asarray(A).astype(dtype)
    y = np.asarray(y).astype(dtype)
    theta = np.asarray(theta).astype(dtype)
    nu64 = np.asarray(nu_draws, dtype=np.float64)
    nu = nu64.astype(dtype)
    const = {v: T.t_constant(v, dtype) for v in np.unique(nu64)}
    c = np.array([const[v] for v in nu64], dtype=dtype)
    sg = theta[:, -1]
    r = y[:, None] - A @ theta[:, :-1].T
    return ((c - np.log(sg))[None, :]
            - ((nu + 1) / 2)[None, :] * np.log1p(r * r / (nu * sg * sg)[None, :]))


def pointwise(A, y, theta, nu_draws, dtype=np.float64):
    """dict of [n] arrays lppd, p_waic, mean_ll (as tscore_reference.pointwise)."""
    S = np.asarray(theta).shape[0]
    with np.errstate(all="ignore"):
        ll = loglik_tv(A, y, theta, nu_draws, dtype)
        return {"lppd": R._lse(ll, 1) - np.log(dtype(S)), "p_waic": ll.var(axis=1, ddof=1),
                "mean_ll": ll.mean(axis=1)}


def loo_pointwise(A, y, theta, nu_draws, dtype=np.float64):
    """dict of [n] arrays elpd_loo, pareto_k, lppd, p_loo (as tscore_reference.loo_pointwise)."""
    n, S = np.asarray(A).shape[0], np.asarray(theta).shape[0]
    out = {key: np.empty(n, dtype=dtype) for key in ("elpd_loo", "pareto_k", "lppd")}
    with np.errstate(all="ignore"):
        ll = loglik_tv(A, y, theta, nu_draws, dtype)
        out["lppd"][:] = R._lse(ll, 1) - np.log(dtype(S))
    for r in range(n):
        if not np.isfinite(ll[r]).all():
            out["elpd_loo"][r] = out["pareto_k"][r] = np.nan
            continue
        out["elpd_loo"][r], out["pareto_k"][r] = PR.psis_row(ll[r], dtype)
    out["p_loo"] = out["lppd"] - out["elpd_loo"]
    return out


# ---- the cases of test_tscore_nu_gpu.py (seeded; no GPU) ---------------------------------------------
# tscore_reference.shape_case problems: points on both sides of the 64-wide tile; 25 draws is the
# smallest number that is smoothed, 130 crosses two 64-draw tiles
SHAPES = tuple((4, n, S) for n in (63, 65) for S in (25, 130))
CYCLE = (1.5, 4.0, 50.0)


def cycling_nu(S):
    return np.array([CYCLE[s % 3] for s in range(S)])


@functools.lru_cache(maxsize=None)
def reference(k, n, S, dtype=np.float64):
    """(pointwise, loo_pointwise) of a shape case with nu cycling over the draws, computed once."""
    A, y, th = T.shape_case(k, n, S)
    nu = cycling_nu(S)
    return pointwise(A, y, th, nu, dtype), loo_pointwise(A, y, th, nu, dtype)


# ---- bars, by the rule of tscore_reference.BAR_*: 100 x the float64 floor of this reference against
# long double on these very cases (test_tscore_nu_host.py re-measures the floors) ----------------------
BAR_LPPD = T.BAR_LPPD     # 1e-11 max(1, |ref|), the bar of test_scoring_gpu.py
BAR_REL = T.BAR_REL       # p_waic_i and mean_ll_i, relative, the same
FLOOR_ELPD = 9.0e-16      # |d elpd_loo_i| / max(1, |ref|) of float64 against long double, measured
FLOOR_K = 3.4e-15         # |d pareto_k|, where finite, measured
BAR_ELPD = 100 * FLOOR_ELPD
BAR_K = 100 * FLOOR_K
