"""Dense numpy restatement of the leave-one-out predictive moments under the Student-t likelihood
(``nu=`` / ``nu_draws=`` of pybmc_amd.scoring.psis_loo_predict): the estimator of
loo_predict_reference.py (its weights_row: PSIS weights, ties shared) with the marginal t density of
tscore_reference / tscore_nu_reference, the t distribution function in place of Phi and the t
variance rule.  Everything in ``dtype``: float64 (the distribution function is scipy.special.stdtr),
or np.longdouble for the rounding floor (a continued fraction of its own, modified Lentz, which
test_loo_predict_t_host.py pins to mpmath).

Per point, with nu_s the draw's degrees of freedom, r_s = y - a . beta_s, z_s = r_s / sigma_s:
loo_mean = y - sum w r; loo_sd = sqrt(sum w (sigma^2 nu / (nu - 2) + r^2) - (sum w r)^2) when every
nu_s > 2, else +inf wherever ll is finite; loo_pit = sum w F_nu(z); ess = 1 / sum w^2.
TEST INFRASTRUCTURE ONLY; shared by test_loo_predict_t_host.py and test_loo_predict_t_gpu.py."""
import numpy as np
from scipy.special import stdtr

import loo_predict_reference as L
import psis_reference as P
import score_reference as R
import tscore_nu_reference as TV
import tscore_reference as T

KEYS, NEW_KEYS = L.KEYS, L.NEW_KEYS
NU_RANGE = (0.06, 1000.0)
# the grid of the distribution-function checks (host: g++ build; GPU: the device's values)
CDF_NUS = (0.06, 0.3, 1.0, 1.5, 2.0, 2.5, 4.0, 17.3, 50.0, 100.0, 1000.0)
CDF_SPECIAL = (0.0, 1e-20, 1e-8, 0.5, 3.0, 40.0, 1e3, 1e6)

# The rounding floors of this reference, float64 against np.longdouble, over every case of
# test_loo_predict_t_gpu.py (all_cases(); measured by test_loo_predict_t_host.py, which asserts
# them; rounded up in the second digit): loo_mean, loo_sd, loo_pit absolute, ess relative.
# FLOORS_BIG: the points whose reference pareto_k exceeds 1.  The GPU bars are 100 x these.
# loo_mean and loo_sd are set by the planted outlier of tscore_reference.outlier_case (a residual of
# 40 units, so sums 1600 times the size of the other points'): under nu = 1.5 .. 4 its pareto_k stays
# below 1, so it counts among the ordinary points here, where the Gaussian reference has it in the
# k > 1 class.  Without that point the largest are 5.5e-16 and 6.3e-16.
FLOORS = {"loo_mean": 9.4e-15, "loo_sd": 1.7e-13, "loo_pit": 4.6e-16, "ess": 1.7e-15}
FLOORS_BIG = {"loo_mean": 7.9e-15, "loo_sd": 4.6e-13, "loo_pit": 3.4e-16, "ess": 3.8e-15}


# ---- the distribution function ----------------------------------------------------------------------
def _betacf(a, b, x, dtype):
    """The continued fraction of the incomplete beta function I_x(a, b) by modified Lentz
    (Numerical Recipes 6.4), elementwise in ``dtype``: I_x = x^a (1 - x)^b / (a B(a, b)) times this."""
    tiny = np.finfo(dtype).tiny * dtype(1e30)
    eps = np.finfo(dtype).eps

    def guard(v):
        return np.where(np.abs(v) < tiny, tiny, v)
    qab, qap, qam = a + b, a + 1, a - 1
    c = np.ones_like(x)
    d = 1 / guard(1 - qab * x / qap)
    h = d.copy()
    for m in range(1, 2000):
        m2 = 2 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1 / guard(1 + aa * d)
        c = guard(1 + aa / c)
        h = h * d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1 / guard(1 + aa * d)
        c = guard(1 + aa / c)
        de = d * c
        h = h * de
        if not np.any(np.abs(de - 1) > eps):     # (NaN counts as done)
            break
    return h


def t_cdf(z, nu, dtype=np.float64):
    """F_nu(z) elementwise (nu broadcast to z); float64: scipy's stdtr."""
    if dtype == np.float64:
        return stdtr(np.asarray(nu, dtype=np.float64), np.asarray(z, dtype=np.float64))
    z = np.asarray(z, dtype=dtype)
    nu64 = np.broadcast_to(np.asarray(nu, dtype=np.float64), z.shape)
    nu = nu64.astype(dtype)
    const = {v: T.t_constant(v, dtype) for v in np.unique(nu64)}
    c = np.vectorize(const.get, otypes=[dtype])(nu64) if nu64.size else nu
    half = dtype(1) / 2
    with np.errstate(all="ignore"):
        az = np.abs(z)
        u = az * az / nu
        x = 1 / (1 + u)
        zf = az * np.exp(c - (nu + 1) / 2 * np.log1p(u))
        centre = u <= 3 / (nu + 2)
        a = np.where(centre, half, nu / 2)
        b = np.where(centre, nu / 2, half)
        cf = _betacf(a, b, np.where(centre, u * x, x), dtype)
        q = np.where(centre, half - zf * cf, zf * cf / nu)
        q = np.where(np.isinf(u), dtype(0), q)
        return np.where(z < 0, q, 1 - q)


# ---- the estimator ----------------------------------------------------------------------------------
def nu_of_draws(S, nu=None, nu_draws=None):
    """[S] float64: every draw's degrees of freedom."""
    assert (nu is None) != (nu_draws is None)
    return np.full(S, float(nu)) if nu_draws is None else np.asarray(nu_draws, dtype=np.float64).reshape(-1)


def loglik(A, y, theta, nu=None, nu_draws=None, dtype=np.float64):
    if nu_draws is None:
        return T.loglik_t(A, y, theta, nu, dtype)
    return TV.loglik_tv(A, y, theta, np.asarray(nu_draws).reshape(-1), dtype)


def pointwise(A, y, theta, nu=None, nu_draws=None, dtype=np.float64, ties="share", chunk=64):
    """dict of [n] arrays KEYS (a point with a non-finite ll: NaN in all but lppd)."""
    A = np.asarray(A).astype(dtype)
    y = np.asarray(y).astype(dtype)
    th = np.asarray(theta).astype(dtype)
    n, S = A.shape[0], th.shape[0]
    nus64 = nu_of_draws(S, nu, nu_draws)
    nus = nus64.astype(dtype)
    sg = th[:, -1]
    sd_inf = bool(np.any(nus64 <= 2))
    with np.errstate(all="ignore"):
        var = np.zeros(S, dtype=dtype) if sd_inf else sg * sg * (nus / (nus - 2))
    out = {key: np.full(n, np.nan, dtype=dtype) for key in KEYS}
    for i0 in range(0, n, chunk):
        sl = slice(i0, min(n, i0 + chunk))
        with np.errstate(all="ignore"):
            ll = loglik(A[sl], y[sl], th, nu, nu_draws, dtype)
            out["lppd"][sl] = R._lse(ll, 1) - np.log(dtype(S))
            r = y[sl, None] - A[sl] @ th[:, :-1].T
            ok = np.isfinite(ll).all(axis=1)
            F = np.full(ll.shape, np.nan, dtype=dtype)
            if ok.any():
                F[ok] = t_cdf(r[ok] / sg[None, :], nus64[None, :], dtype)
        for j in range(ll.shape[0]):
            if not ok[j]:
                continue
            W, elpd, khat = L.weights_row(ll[j], dtype, ties)
            w = W / W.sum()
            mr = (w * r[j]).sum()
            i = i0 + j
            out["elpd_loo"][i], out["pareto_k"][i] = elpd, khat
            out["loo_mean"][i] = y[i] - mr
            out["loo_sd"][i] = np.inf if sd_inf else np.sqrt((w * (var + r[j] * r[j])).sum() - mr * mr)
            out["loo_pit"][i] = (w * F[j]).sum()
            out["ess"][i] = 1 / (w * w).sum()
    return out


# ---- the cases of test_loo_predict_t_gpu.py (seeded; no GPU) ----------------------------------------
NUS = T.NUS                        # 1.5, 4, 50
CYCLE_INF = (1.5, 4.0, 50.0)       # a nu per draw with one at or below 2: loo_sd = +inf
CYCLE_FINITE = (2.5, 4.0, 50.0)


def cycling(S, values):
    return np.array([values[s % len(values)] for s in range(S)])


def ties_case():
    """The S / 2 ties of test_loo_predict_gpu.py."""
    A, y, th = R.random_case(200, 5, 9000, 77)
    rng = np.random.default_rng(3)
    rep = th[0].copy()
    rep[:5] += 0.5
    t2 = th.copy()
    t2[rng.permutation(9000)[:4500]] = rep
    return A, y, t2


def base_cases():
    """(tag, (A, y, theta)) of tscore_reference's cases."""
    for tag, kind, key in T.all_cases():
        yield tag, T.case_arrays(kind, key)


def lik_of(spec, S):
    """The likelihood keywords of a spec: a number (nu), or a tuple of values cycling over the draws."""
    return {"nu_draws": cycling(S, spec)} if isinstance(spec, tuple) else {"nu": float(spec)}


def grouped_cases():
    """(group, tag, (A, y, theta), spec) of every parity case the GPU file checks against this
    reference; the group names the GPU test that runs it."""
    for tag, arrays in base_cases():
        for nu in NUS:
            yield f"tscore nu={nu:g}", f"{tag} nu={nu:g}", arrays, nu
    for spec in (CYCLE_INF, CYCLE_FINITE, 2.0, 2.5):
        for k, n, S in TV.SHAPES + ((4, 130, 4097),):
            yield f"spec {spec}", f"k={k} n={n} S={S} nu={spec}", T.shape_case(k, n, S), spec
        yield f"spec {spec}", f"outlier nu={spec}", T.outlier_case(), spec
    for k, spec in ((3, 4.0), (33, CYCLE_FINITE)):
        for case, n, S, arrays in P.shape_cases(k):
            yield f"shapes k={k}", f"shape k={k} n={n} S={S} nu={spec}", arrays, spec
    yield "ties", "ties nu=4", ties_case(), 4.0
    yield "mirror", "mirror nu=4", L.mirror_case(), 4.0
    yield "mirror", f"mirror nu={CYCLE_FINITE}", L.mirror_case(), CYCLE_FINITE


def all_cases():
    """(tag, (A, y, theta), spec) of grouped_cases()."""
    for _, tag, arrays, spec in grouped_cases():
        yield tag, arrays, spec


def group(name):
    """The (tag, (A, y, theta), spec) of one group."""
    return [(tag, arrays, spec) for g, tag, arrays, spec in grouped_cases() if g == name]


_REFERENCES = {}


def reference(tag, arrays=None, spec=None):
    """The float64 reference of a case of grouped_cases(), computed once per session (from `arrays`
    and `spec` when the caller has them at hand); not to be modified."""
    if tag not in _REFERENCES:
        if arrays is None:
            arrays, spec = next((a, sp) for t, a, sp in all_cases() if t == tag)
        A, y, th = arrays
        _REFERENCES[tag] = pointwise(A, y, th, **lik_of(spec, len(th)))
    return _REFERENCES[tag]
