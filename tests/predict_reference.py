"""Host mirrors of the posterior predictive leg (pybmc_amd/csrc/kernels_predict.hip), in numpy.

  requested_ranks(S, q, cov)    the ranks a call asks of every point, as the kernels list them
  selection_route(row, ranks)   what predict_select_kernel does with one point's draws: "flat",
                                "unusable", "select" or "fallback" -- the same IEEE operations and
                                the constants of bmc_plan.h (tests/test_predict_plan.py compares them
                                with what tests/predict_plan_check.cpp prints)
  expected_bands(draws, qi, qg) sort + the kernels' interpolation
  predictive_reference(...)     the draws in extended precision and the derived error bar
"""
import math

import numpy as np

from pybmc_amd._lib import coverage_plan, order_stat_plan

SEL_BINS, SEL_CAP, SEL_THREADS = 4096, 64, 512


def requested_ranks(S, q, cov_percentiles):
    """Percentile neighbours (lo, min(lo + 1, S - 1)) then coverage bounds (lo, hi)."""
    ranks = []
    qi, _ = order_stat_plan(S, q)
    for lo in qi:
        ranks += [int(lo), min(int(lo) + 1, S - 1)]
    if cov_percentiles is not None:
        lo, hi = coverage_plan(S, cov_percentiles)
        for a, b in zip(lo, hi):
            ranks += [int(a), int(b)]
    return ranks


def selection_route(row, ranks):
    """The branch predict_select_kernel takes for one point (finite draws)."""
    row = np.asarray(row, dtype=np.float64)
    mn, mx = row.min(), row.max()
    if mx == mn:
        return "flat"
    with np.errstate(over="ignore", divide="ignore"):
        scale = np.float64(SEL_BINS) / (mx - mn)
    if not (scale > 0.0 and scale < 1.7e308):
        return "unusable"
    t = (row - mn) * scale                       # two roundings, as the kernel (no contraction)
    b = np.clip(t.astype(np.int64), 0, SEL_BINS - 1)      # (int) truncates; t >= 0 here
    hist = np.bincount(b, minlength=SEL_BINS)
    cum = np.cumsum(hist)
    # the bin of rank r: the first whose inclusive prefix exceeds r (never an empty one)
    bins = np.searchsorted(cum, np.asarray(ranks, dtype=np.int64), side="right")
    return "fallback" if (hist[bins] > SEL_CAP).any() else "select"


def expected_bands(draws, qi, qg):
    """numpy's linear method as the kernels evaluate it, on sorted columns of (S, M) draws."""
    srt = np.sort(np.asarray(draws), axis=0)
    S = srt.shape[0]
    out = np.empty((len(qi), srt.shape[1]))
    for j, (lo, t) in enumerate(zip(qi, qg)):
        a, b = srt[lo], srt[min(lo + 1, S - 1)]
        d = b - a
        out[j] = b - d * (1.0 - t) if t >= 0.5 else a + d * t
    return out


def longdouble_is_extended():
    return np.finfo(np.longdouble).nmant == 63


def _two_product(a, b):
    """a * b = p + e exactly (Dekker / Veltkamp; no overflow or underflow at the test's sizes)."""
    p = a * b
    c = 134217729.0   # 2^27 + 1
    ah = a * c
    ah = ah - (ah - a)
    al = a - ah
    bh = b * c
    bh = bh - (bh - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _reference_fsum(preds, theta, Vt, noise):
    """Exactly rounded sums of exact products; the weights carried as hi + lo pairs."""
    M, Km = preds.shape
    S, k = theta.shape[0], theta.shape[1] - 1
    w0 = 1.0 / Km
    w0_lo = (1.0 - w0 * Km) / Km                    # 1 / Km = w0 + w0_lo to ~2^-106
    Whi, Wlo = np.empty((S, Km)), np.empty((S, Km))
    for s in range(S):
        p, e = _two_product(theta[s, :k, None], Vt)          # (k, Km)
        for m in range(Km):
            terms = list(p[:, m]) + list(e[:, m]) + [w0, w0_lo]
            hi = math.fsum(terms)
            Whi[s, m] = hi
            Wlo[s, m] = math.fsum(terms + [-hi])
    ref = np.empty((S, M), dtype=np.longdouble)
    for s in range(S):
        zp, ze = _two_product(noise[s], np.full(M, theta[s, k]))
        for pt in range(M):
            p, e = _two_product(preds[pt], Whi[s])
            terms = list(p) + list(e) + list(preds[pt] * Wlo[s]) + [zp[pt], ze[pt]]
            hi = math.fsum(terms)
            ref[s, pt] = np.longdouble(hi) + np.longdouble(math.fsum(terms + [-hi]))
    return ref


def predictive_reference(preds, theta, Vt, noise, force_fsum=False):
    """(ref, bar), both (S, M).  ref[s, p] = sum_m preds[p, m] (sum_i theta[s, i] Vt[i, m] + 1 / Km)
    + noise[s, p] theta[s, k] in extended precision (numpy's 80-bit long double where it has a
    64-bit mantissa, otherwise exactly rounded sums of exact products), and the bar every float64
    evaluation must meet whatever its order of summation:
        (Km + k + 4) 2^-53 (sum_m |p_m| (sum_i |theta_i V_im| + 1 / Km) + |z| sigma)."""
    preds = np.asarray(preds, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    Vt = np.asarray(Vt, dtype=np.float64)
    noise = np.asarray(noise, dtype=np.float64)
    Km, k = preds.shape[1], Vt.shape[0]
    L = np.longdouble
    if longdouble_is_extended() and not force_fsum:
        W = theta[:, :k].astype(L) @ Vt.astype(L) + L(1) / L(Km)
        ref = W @ preds.T.astype(L) + noise.astype(L) * theta[:, k].astype(L)[:, None]
    else:
        ref = _reference_fsum(preds, theta, Vt, noise)
    absW = np.abs(theta[:, :k]).astype(L) @ np.abs(Vt).astype(L) + L(1) / L(Km)
    mag = absW @ np.abs(preds).T.astype(L) + np.abs(noise).astype(L) * np.abs(theta[:, k]).astype(L)[:, None]
    bar = L(Km + k + 4) * L(2.0) ** -53 * mag
    return ref, bar
