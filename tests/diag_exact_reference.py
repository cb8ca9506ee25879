"""Plain numpy longdouble references of what the chain-diagnostics kernels compute before the host's
ESS scan sees it (kernels_diag.hip through bmc_chain_autocov): per split half-chain the mean of
x - shift and the centred sum of squares M2, and a(t) = mean over the 2C halves of
(1/n) sum_{i < n-t} d_i d_{i+t}.  Direct sums, no FFT, and beside every value a running bound on
|computed - exact| for a correct float64 evaluation, from the standard model
fl(a op b) = (a op b)(1 + delta), |delta| <= u = 2^-53 (fma: one rounding), gamma_q = q u / (1 - q u).

With y_i = x_i - shift (shift = the column's first kept draw of chain 0), mu = mean_i y_i and
d_i = y_i - mu of one half-chain of n draws:

mean   The kernels form fl(x_i - shift) (one rounding each), add n of them in some order, divide by
       the count and merge the row splits by count-weighted updates: at most n + 8 roundings lie
       behind any term whatever the order, so |mu_c - mu| <= dmu = gamma_{n+8} mean_i |y_i|.
d_i    d_c = fl(fl(x_i - shift) - mu_c): |d_c - d_i| <= e_i = u |y_i| + u |d_i| + dmu (first order:
       the dropped terms are u times these).
M2,    A sum of products of perturbed factors: each product is off by at most
acov   |d_i| e_{i+t} + e_i |d_{i+t}| + e_i e_{i+t} (t = 0 for M2), and the summation itself (an fma
       chain, the fixed-order sum of the workgroups' partials, the divisions by n and 2C) by at most
       gamma_q sum_i |d_i d_{i+t}| when no term passes through more than q roundings;
       q = n + 2C + 16 covers a half-chain's n fmas, a sum over the 2C halves and the fixed
       steps.  M2's bound is that sum; a(t)'s is the sum divided by n, averaged over the halves.
       (M2 is computed per row split about the split's own mean and merged: the exact result is
       the same, the split sums of squares are no larger, and the merge's delta^2 na nb / (na + nb)
       terms err by at most 2 |delta| dmu na nb / (na + nb) <= dmu sum_i |d_i|, which the e_i hold.)
       One evaluation is outside the premise: a workgroup that owns spg > 1 half-chains chains
       spg n fmas behind the first one's terms, more than q when (spg - 1) n > 2C + 16.  The
       first-order model still bounds it by gamma_{spg n + ...}; the class tests print how far
       below 1 the measured ratios of those shapes stay.

A lag t >= n has no terms: value 0, bound 0.  The references' own error is a few 2^-64 relative
(numpy sums the contiguous axis pairwise), three orders below the bounds; the bounds' own sums of
non-negative terms are taken in float64 and inflated by 2^-20."""
import numpy as np

from setup_reference import LD, U, gamma, worst_ratio  # noqa: F401  (worst_ratio: for the tests)

INFLATE = 1.0 + 2.0 ** -20


def split(x, burn=0):
    """(halves (2C, n, P) float64, middle (C, P) or None, shift (P,)) of samples (C, T, P) or (T, P):
    sequence 2c + h is half h of chain c."""
    a = np.asarray(x, dtype=np.float64)
    a = a if a.ndim == 3 else a[None]
    C, T, P = a.shape
    kept = a[:, burn:]
    Tp = T - burn
    n = Tp // 2
    assert n >= 4
    halves = np.stack([kept[:, :n], kept[:, Tp - n:]], axis=1).reshape(2 * C, n, P)
    middle = kept[:, n].copy() if Tp & 1 else None
    return halves, middle, kept[0, 0].copy()


def exact(x, burn=0, cols=None, first_lag=0, n_lags=64):
    """Dict of longdouble arrays: seq_mean, seq_m2 (2C, P) with their bounds dmean, dm2; acov
    (len(cols), n_lags) with dacov; and shift (P,) float64, n, and q."""
    halves, _, shift = split(x, burn)
    M, n, P = halves.shape
    cols = np.arange(P) if cols is None else np.asarray(cols)
    q = n + M + 16
    y = halves.astype(LD) - shift.astype(LD)
    ya = np.abs(y)
    mu = y.sum(1) / n
    dmu = gamma(n + 8) * (ya.sum(1) / n)
    d = y - mu[:, None, :]
    da = np.abs(d)
    e = U * ya + U * da + dmu[:, None, :]
    m2 = (d * d).sum(1)
    dm2 = gamma(q) * m2 + (2 * da * e + e * e).sum(1)

    dc = np.ascontiguousarray(d[:, :, cols].transpose(0, 2, 1))              # (M, A, n): sums pairwise
    ac = np.ascontiguousarray(da[:, :, cols].transpose(0, 2, 1)).astype(np.float64)
    ec = np.ascontiguousarray(e[:, :, cols].transpose(0, 2, 1)).astype(np.float64)
    gc = ac + ec
    gq = float(gamma(q))
    acov = np.zeros((len(cols), n_lags), LD)
    dacov = np.zeros((len(cols), n_lags), LD)
    for k in range(n_lags):
        t = first_lag + k
        if t >= n:
            break
        s = (dc[..., :n - t] * dc[..., t:]).sum(-1)
        b = gq * np.einsum("mai,mai->ma", ac[..., :n - t], ac[..., t:])
        b += np.einsum("mai,mai->ma", ac[..., :n - t], ec[..., t:])
        b += np.einsum("mai,mai->ma", ec[..., :n - t], gc[..., t:])
        acov[:, k] = s.sum(0) / n / M
        dacov[:, k] = (b * INFLATE).astype(LD).sum(0) / n / M
    return dict(seq_mean=mu, dmean=dmu, seq_m2=m2, dm2=dm2, acov=acov, dacov=dacov, shift=shift, n=n, q=q)


def float64_evaluation(x, burn=0, cols=None, first_lag=0, n_lags=64):
    """The same quantities by numpy in float64 (pairwise sums: another correct order)."""
    halves, _, shift = split(x, burn)
    M, n, P = halves.shape
    cols = np.arange(P) if cols is None else np.asarray(cols)
    y = halves - shift
    mu = y.mean(1)
    d = y - mu[:, None, :]
    dc = np.ascontiguousarray(d[:, :, cols].transpose(0, 2, 1))
    acov = np.zeros((len(cols), n_lags))
    for k in range(n_lags):
        t = first_lag + k
        if t >= n:
            break
        acov[:, k] = ((dc[..., :n - t] * dc[..., t:]).sum(-1) / n).mean(0)
    return dict(seq_mean=mu, seq_m2=(d * d).sum(1), acov=acov)
