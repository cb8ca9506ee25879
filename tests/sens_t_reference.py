"""Dense numpy restatement of the power-scaling sensitivity of a Student-t fit (pybmc_amd/sensitivity.py
states the model): the log densities under the t likelihood, nu fixed or one per draw, and the log
prior of nu.  Everything downstream of a log-density vector -- the Pareto-smoothed weights, the
distance, the quantity columns, psens, the reading -- is tests/sens_reference.py's, imported, not
restated.  Everything in ``dtype``: float64, or np.longdouble for the rounding floor; the t
constant comes from tests/tscore_reference.py (long double whatever ``dtype`` is).  TEST
INFRASTRUCTURE ONLY."""
import numpy as np

import sens_reference as SR
from sens_reference import cjs_distance, diagnose, psens, psis_weights, quantities   # noqa: F401
from tscore_reference import t_constant

T_COMPONENTS = SR.COMPONENTS + ("prior_nu",)


def _nu_per_draw(nu, S, dtype):
    """(nu_s [S], lp_nu [S]) of ``nu``: a number, or (values, index, log_prior or None)."""
    if isinstance(nu, tuple):
        values, index, log_prior = nu
        values = np.asarray(values, dtype=np.float64)
        index = np.asarray(index)
        assert index.shape == (S,) and index.min() >= 0 and index.max() < len(values)
        lp = np.zeros(len(values)) if log_prior is None else np.asarray(log_prior)
        return values, index, np.asarray(lp).astype(dtype)[index]
    return np.array([float(nu)]), np.zeros(S, dtype=np.int64), np.zeros(S, dtype=dtype)


def log_densities_t(A, y, theta, prior, nu, dtype=np.float64):
    """(lp_beta, lp_sigma2, loglik, lp_nu), each [S].  ``nu``: the degrees of freedom of every draw,
    or (values, index, log_prior): draw s has values[index[s]] and lp_nu = log_prior[index[s]]
    (log_prior None: 0).  NaN, all four, for a draw with a non-finite coefficient or without a
    finite sigma > 0."""
    lp_beta, lp_sigma2, _ = SR.log_densities(A, y, theta, prior, dtype)
    A = np.asarray(A, dtype=dtype)
    y = np.asarray(y, dtype=dtype)
    theta = np.asarray(theta, dtype=dtype)
    N, k = A.shape
    S = theta.shape[0]
    values, index, lp_nu = _nu_per_draw(nu, S, dtype)
    nus = values.astype(dtype)[index]
    const = np.array([t_constant(v, dtype) for v in values], dtype=dtype)[index]
    beta, sigma = theta[:, :k], theta[:, k]
    with np.errstate(all="ignore"):
        res = y[None, :] - beta @ A.T
        terms = np.log1p(res * res / (nus * sigma * sigma)[:, None])
        loglik = N * (const - np.log(sigma)) - (nus + 1) / 2 * terms.sum(axis=1)
    bad = ~(np.isfinite(theta).all(axis=1) & (sigma > 0))
    loglik[bad] = np.nan
    lp_nu = lp_nu.copy()
    lp_nu[bad] = np.nan
    return lp_beta, lp_sigma2, loglik, lp_nu


def component_vector(lp, name):
    lb, ls, ll, ln = lp
    return {"prior": lb + ls + ln, "likelihood": ll, "prior_beta": lb, "prior_sigma2": ls, "prior_nu": ln}[name]


def quantities_t(theta, Vt, nu, dtype=np.float64):
    """sens_reference.quantities and, with a nu per draw, one more column, the last: nu_s."""
    X = quantities(theta, Vt, dtype)
    if isinstance(nu, tuple):
        values, index, _ = nu
        X = np.concatenate([X, np.asarray(values, dtype=dtype)[np.asarray(index)][:, None]], axis=1)
    return X


def sensitivity(A, y, theta, prior, nu, Vt=None, alphas=(0.99, 1.01), components=("prior", "likelihood"),
                dtype=np.float64):
    """sens_reference.sensitivity under the t likelihood: the same dict, lp (4, S)."""
    lp = log_densities_t(A, y, theta, prior, nu, dtype)
    X = quantities_t(theta, Vt, nu, dtype)
    S, Qn = X.shape
    nc, na = len(components), len(alphas)
    out = {"lp": np.stack(lp), "weights": np.full((nc, na, S), np.nan, dtype=dtype),
           "pareto_k": np.full((nc, na), np.nan, dtype=dtype)}
    for key in ("mean", "sd", "cjs"):
        out[key] = np.full((nc, na, Qn), np.nan, dtype=dtype)
    col_ok = np.isfinite(X).all(axis=0)
    out["column_flags"] = ~col_ok
    out["component_flags"] = np.zeros(nc, dtype=bool)
    for ci, c in enumerate(components):
        v = component_vector(lp, c)
        if not np.isfinite(v).all():
            out["component_flags"][ci] = True
            continue
        for ai, a in enumerate(alphas):
            w, kh = psis_weights(v, a, dtype)
            out["weights"][ci, ai] = w
            out["pareto_k"][ci, ai] = kh
            for q in range(Qn):
                if col_ok[q]:
                    out["cjs"][ci, ai, q], out["mean"][ci, ai, q], out["sd"][ci, ai, q] = \
                        cjs_distance(X[:, q], w, dtype)
    return out


def nu_table(nu_draws):
    """(values, index) of per-draw nu, as the library tabulates them."""
    values, index = np.unique(np.asarray(nu_draws, dtype=np.float64), return_inverse=True)
    return values, index.reshape(-1)


def log_prior_of(values, grid, weight, dtype=np.float64):
    """log(w_g / sum w) of every value, each a value of ``grid``."""
    grid = np.asarray(grid, dtype=np.float64)
    at = np.array([int(np.flatnonzero(grid == v)[0]) for v in values])
    w = np.asarray(weight).astype(dtype)
    return np.log(w[at] / w.sum())
