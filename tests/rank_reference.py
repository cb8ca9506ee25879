"""Plain numpy / scipy restatement of the rank-normalised diagnostics (pybmc_amd/rankdiag.py
docstring; Vehtari et al. 2021): scipy.stats.rankdata(method="average") for the ranks,
scipy.special.ndtri for the z-scores, np.quantile(method="linear") for the quantiles, and the
split R-hat / ESS of tests/diag_reference.py for R and E."""
import numpy as np
from scipy.special import ndtri
from scipy.stats import rankdata

import diag_reference as R

SERIES = ("z", "zf", "lo", "hi")       # z(x), z(|x - med|), 1[x <= q05], 1[x <= q95]


def split(samples, burn=0):
    """(2C, n, P) split draws of a (T, P) or (C, T, P) array: sequence 2c + h is half h of chain c."""
    a = np.asarray(samples, dtype=np.float64)
    if a.ndim == 2:
        a = a[None]
    C, T, P = a.shape
    Tp = T - burn
    n = Tp // 2
    assert n >= 4
    kept = a[:, burn:]
    return np.stack([kept[:, :n], kept[:, Tp - n:]], axis=1).reshape(2 * C, n, P)


def z_scores(v):
    """Rank normalisation of every column of a (M, n, P) array over its M n values."""
    M, n, P = v.shape
    S = M * n
    out = np.empty_like(v)
    for j in range(P):
        col = v[:, :, j].reshape(-1) + 0.0          # (-0.0 + 0.0 = +0.0: equality by value)
        r = rankdata(col, method="average")
        out[:, :, j] = ndtri((r - 0.375) / (S + 0.25)).reshape(M, n)
    return out


def rank_normalize(samples, burn=0, folded=False):
    x = split(samples, burn)
    if folded:
        M, n, P = x.shape
        med = np.quantile(x.reshape(M * n, P), 0.5, axis=0, method="linear")
        x = np.abs(x - med)
    return z_scores(x)


def derived(samples, burn=0):
    """The four derived series of every column, dict name -> (2C, n, P), and the tail quantiles."""
    x = split(samples, burn)
    M, n, P = x.shape
    flat = x.reshape(M * n, P)
    q05, med, q95 = np.quantile(flat, [0.05, 0.5, 0.95], axis=0, method="linear")
    return dict(z=z_scores(x), zf=z_scores(np.abs(x - med)), lo=(x <= q05).astype(np.float64),
                hi=(x <= q95).astype(np.float64)), q05, q95


def _classic(series):
    """R, E and the stopping pair sum of every column of a (M, n, P) series."""
    M, n, P = series.shape
    rhat, ess, stop = np.full(P, np.nan), np.full(P, np.nan), np.full(P, np.nan)
    for j in range(P):
        x = series[:, :, j]
        means = x.mean(1)
        W = x.var(1, ddof=1).mean()
        if W == 0:
            continue
        var_plus = (n - 1) / n * W + means.var(ddof=1)
        rhat[j] = np.sqrt(var_plus / W)
        acov = R.autocov_fft(x - means[:, None]).mean(0)
        ess[j], t = R.ess_scan(acov, W, var_plus, n, M)
        # the pair (re, ro) the scan held when its loop ended: rho(t - 1), rho(t) (re = 1 at t = 1)
        rho = 1.0 - (W - acov) / var_plus
        stop[j] = (1.0 if t == 1 else rho[t - 1]) + rho[t]
    return rhat, ess, stop


def diagnostics(samples, burn=0, probs=(0.05, 0.5, 0.95)):
    """Dict as pybmc_amd.rank_diagnostics returns it, plus "stop": (4, P) stopping pair sums of the
    ESS scans of the four derived series and "counts": (2, P) sums of the two indicators."""
    a = np.asarray(samples, dtype=np.float64)
    classic = R.diagnostics(a, burn=burn)
    x = split(a, burn)
    M, n, P = x.shape
    flat = x.reshape(M * n, P)
    bad = ~np.isfinite(flat).all(0)
    safe = np.where(bad[None, None, :], 0.0, x)
    der, _, _ = derived(safe.reshape(M // 2, 2 * n, P))
    res = {k: _classic(der[k]) for k in SERIES}
    with np.errstate(invalid="ignore"):
        r_hat = np.maximum(res["z"][0], res["zf"][0])          # NaN when either is
        ess_tail = np.minimum(res["lo"][1], res["hi"][1])
        quant = np.quantile(np.where(bad[None, :], 0.0, flat), np.asarray(probs, dtype=np.float64), axis=0,
                            method="linear")
    ess_bulk = res["z"][1].copy()
    for arr in (r_hat, ess_tail, ess_bulk):
        arr[bad] = np.nan
    quant[:, bad] = np.nan
    with np.errstate(invalid="ignore", divide="ignore"):
        mcse = classic["sd"] / np.sqrt(ess_bulk)
    return dict(mean=classic["mean"], sd=classic["sd"], mcse_mean=mcse, ess_bulk=ess_bulk, ess_tail=ess_tail,
                r_hat=r_hat, quantiles=quant, stop=np.stack([res[k][2] for k in SERIES]),
                counts=np.stack([der["lo"].sum((0, 1)), der["hi"].sum((0, 1))]))
