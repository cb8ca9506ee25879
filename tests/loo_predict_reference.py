"""Dense numpy restatement of the leave-one-out predictive moments of
pybmc_amd.scoring.psis_loo_predict, written from the estimator's definition on top of
psis_reference (tail length, generalised Pareto fit) and score_reference (ll).  Everything in
``dtype`` (float64, or np.longdouble for the rounding floor).

Per point, over the S draws: the weights W_s = exp(lw_s) of PSIS (smoothed for the M tail ranks,
raw elsewhere, truncated at 0); draws with equal ll (equal as numbers) each get the mean W of the
ranks their run occupies; w = W / sum W; r_s = y - a . beta_s;
loo_mean = y - sum w r, loo_sd = sqrt(sum w (sigma^2 + r^2) - (sum w r)^2),
loo_pit = sum w Phi(r / sigma), ess = 1 / sum w^2."""
import numpy as np
from scipy.special import erfc as _erfc64

import psis_reference as P
import score_reference as R

KEYS = ("elpd_loo", "pareto_k", "lppd", "loo_mean", "loo_sd", "loo_pit", "ess")
NEW_KEYS = KEYS[3:]

# The rounding floors of this reference, float64 against np.longdouble, over every case of
# test_loo_predict_gpu.py (measured by test_loo_predict_host.py, which asserts them; rounded up in
# the second digit): loo_mean, loo_sd, loo_pit absolute, ess relative.  FLOORS_BIG: the points whose
# reference pareto_k exceeds 1.  The GPU bars are 100 x these.
FLOORS = {"loo_mean": 1.1e-15, "loo_sd": 3.0e-15, "loo_pit": 4.2e-16, "ess": 5.7e-15}
FLOORS_BIG = {"loo_mean": 1.5e-15, "loo_sd": 6.2e-14, "loo_pit": 2.3e-16, "ess": 2.1e-14}


def _pi(dtype):
    return 4 * np.arctan(dtype(1))     # (np.pi is a float64)


def _erfc_series(ax):
    """erfc of 0 <= ax < 6.6 in ax's dtype: 1 - erf with the all-positive series
    erf(x) = 2 / sqrt(pi) exp(-x^2) sum_n 2^n x^(2n+1) / (2n+1)!!  (absolute error a few eps)."""
    dt = ax.dtype.type
    x2 = 2 * ax * ax
    term = ax.copy()
    s = ax.copy()
    tiny = np.finfo(ax.dtype).eps / 64
    n = 0
    while True:
        term = term * x2 / (2 * n + 3)
        s = s + term
        n += 1
        if not np.any(term > tiny * s) or n > 2000:
            break
    return 1 - 2 / np.sqrt(_pi(dt)) * np.exp(-ax * ax) * s


def erfc(x, dtype=np.float64):
    """erfc(x) elementwise in ``dtype``; scipy's for float64 (which has no extended form)."""
    if dtype == np.float64:
        return _erfc64(np.asarray(x, dtype=np.float64))
    x = np.asarray(x, dtype=dtype)
    ax = np.abs(x)
    out = np.empty_like(ax)
    edges = (0.0, 0.75, 1.5, 2.5, 4.0, 6.6)
    for lo, hi in zip(edges[:-1], edges[1:]):     # (the series' length grows with x^2)
        sel = (ax >= lo) & (ax < hi)
        if sel.any():
            out[sel] = _erfc_series(ax[sel])
    far = ax >= edges[-1]                          # below 4e-20: three terms of the asymptotic series
    if far.any():
        a = ax[far]
        out[far] = np.exp(-a * a) / (a * np.sqrt(_pi(dtype))) * (1 - 1 / (2 * a * a) + 3 / (4 * a ** 4))
    out[np.isnan(x)] = np.nan
    return np.where(x < 0, 2 - out, out)


def phi(z, dtype=np.float64):
    """The standard normal distribution function, erfc(-z / sqrt 2) / 2."""
    z = np.asarray(z, dtype=dtype)
    return erfc(-z / np.sqrt(dtype(2)), dtype) / 2


def weights_row(ll, dtype=np.float64, ties="share"):
    """(W[s] unnormalised, elpd_loo_i, pareto_k) of one point's ll[s].  ties = "share": the
    estimator; "index": the weights as a stable sort hands them to tied draws (NOT the estimator:
    the mirror case tells the two apart)."""
    ll = np.asarray(ll, dtype=dtype)
    S = len(ll)
    lw = -ll
    lw = lw - lw.max()
    M = P.tail_length(S)
    khat = dtype(np.inf)
    if M >= P.MIN_TAIL:
        order = np.argsort(lw, kind="stable")
        tail = order[S - M:]
        cutoff = lw[order[S - M - 1]]
        lt = lw[tail]
        if lt[0] != lt[-1]:
            with np.errstate(all="ignore"):
                ecut = np.exp(cutoff)
                k, sigma = P.gpdfit(np.exp(lt) - ecut, dtype)
                if np.isfinite(k):
                    khat = k
                    p = (np.arange(1, M + 1).astype(dtype) - dtype(0.5)) / M
                    q = -sigma * np.log1p(-p) if abs(k) < 1e-30 else sigma * np.expm1(-k * np.log1p(-p)) / k
                    lw = lw.copy()
                    lw[tail] = np.log(ecut + q)
        lw = np.minimum(lw, 0)
    with np.errstate(all="ignore"):
        a = ll + lw
        elpd = (a.max() + np.log(np.exp(a - a.max()).sum())) - (lw.max() + np.log(np.exp(lw - lw.max()).sum()))
    W = np.exp(lw)
    if ties == "share":
        o = np.argsort(ll, kind="stable")
        v = ll[o]
        starts = np.flatnonzero(np.r_[True, v[1:] != v[:-1]])
        cnt = np.diff(np.r_[starts, S])
        if cnt.max() > 1:
            Ws = W[o]
            mean = np.add.reduceat(Ws, starts) / cnt.astype(dtype)
            shared = np.repeat(mean, cnt)
            Ws = np.where(np.repeat(cnt, cnt) > 1, shared, Ws)
            W = np.empty_like(W)
            W[o] = Ws
    return W, elpd, khat


def pointwise(A, y, theta, dtype=np.float64, ties="share", chunk=64):
    """dict of [n] arrays KEYS (a point with a non-finite ll: NaN in all but lppd)."""
    A = np.asarray(A).astype(dtype)
    y = np.asarray(y).astype(dtype)
    th = np.asarray(theta).astype(dtype)
    n, S = A.shape[0], th.shape[0]
    sg = th[:, -1]
    out = {key: np.full(n, np.nan, dtype=dtype) for key in KEYS}
    for i0 in range(0, n, chunk):
        sl = slice(i0, min(n, i0 + chunk))
        with np.errstate(all="ignore"):
            ll = R.loglik(A[sl], y[sl], th, dtype)
            out["lppd"][sl] = R._lse(ll, 1) - np.log(dtype(S))
            r = y[sl, None] - A[sl] @ th[:, :-1].T
            ph = phi(r / sg[None, :], dtype)
        for j in range(ll.shape[0]):
            if not np.isfinite(ll[j]).all():
                continue
            W, elpd, khat = weights_row(ll[j], dtype, ties)
            w = W / W.sum()
            mr = (w * r[j]).sum()
            i = i0 + j
            out["elpd_loo"][i], out["pareto_k"][i] = elpd, khat
            out["loo_mean"][i] = y[i] - mr
            out["loo_sd"][i] = np.sqrt((w * (sg * sg + r[j] * r[j])).sum() - mr * mr)
            out["loo_pit"][i] = (w * ph[j]).sum()
            out["ess"][i] = 1 / (w * w).sum()
    return out


def summary(y, pw):
    """loo_rmse, pit_coverage (percent, p = 0, 5, .., 100), min_ess."""
    y = np.asarray(y, dtype=np.float64)
    m = np.asarray(pw["loo_mean"], dtype=np.float64)
    dev = np.abs(2 * np.asarray(pw["loo_pit"], dtype=np.float64) - 1)
    return {"loo_rmse": float(np.sqrt(np.mean((y - m) ** 2))),
            "pit_coverage": [100.0 * float(np.mean(dev <= p / 100)) for p in range(0, 101, 5)],
            "min_ess": float(np.min(np.asarray(pw["ess"], dtype=np.float64)))}


def mirror_case(S=9000, n=40, seed=11):
    """k = 3, A[0] = (1, 0, 0), y[0] = 0, S / 2 draws and their copies with beta_0 negated: every
    ll[0, s] occurs twice, with opposite r.  The exact loo_mean[0] is 0 and loo_pit[0] 1/2."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, 3)) / np.sqrt(3)
    A[0] = (1.0, 0.0, 0.0)
    b = np.array([0.0, 0.4, -0.3])
    y = A @ b + 0.2 * rng.standard_normal(n)
    y[0] = 0.0
    half = np.column_stack([b + 0.3 * rng.standard_normal((S // 2, 3)),
                            0.5 + 0.1 * rng.random(S // 2)])
    other = half.copy()
    other[:, 0] = -other[:, 0]
    return A, y, np.concatenate([half, other], axis=0)


def exact_closed_form(A, y, theta, sigma=0.7):
    """(mean, sd, pit) of the exact leave-one-out predictive of P.closed_form_case:
    N(y_i - r_i / (1 - h_i), sigma^2 / (1 - h_i))."""
    h = np.sum(A * A, axis=1)
    r = y - A @ (A.T @ y)
    mean = y - r / (1 - h)
    sd = sigma / np.sqrt(1 - h)
    return mean, sd, phi((y - mean) / sd)
