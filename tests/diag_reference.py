"""Plain-numpy restatement of the convergence diagnostics (pybmc_amd/diagnostics.py docstring;
Vehtari et al. 2021, classic split R-hat and "mean" ESS).  The autocovariances come from a
zero-padded FFT: deliberately not the direct sums the kernels use.  Every column is taken
relative to its first kept draw of chain 0 (the estimator is shift-invariant): a column at 1e4
with sd 1e-2 would otherwise round each sequence mean by ~1e-12, which moves B/n, and so
r_hat, by more than the tests' 1e-12."""
import numpy as np


def autocov_fft(d):
    """acov(t) = (1/n) sum_{i<n-t} d_i d_{i+t} of each row of a centred (M, n) array."""
    n = d.shape[-1]
    nfft = 1 << int(np.ceil(np.log2(2 * n)))
    f = np.fft.rfft(d, nfft, axis=-1)
    return np.fft.irfft(f * np.conj(f), nfft, axis=-1)[..., :n] / n


def ess_scan(a, W, var_plus, n, M):
    """Steps 1-5 of the definition on a(t); returns (ess, max_lag)."""
    def rho_of(t):
        return 1.0 - (W - a[t]) / var_plus

    rho = np.zeros(n)
    rho[0] = 1.0
    re, ro = 1.0, rho_of(1)
    rho[1] = ro
    t = 1
    while t < n - 3 and re + ro > 0:
        re, ro = rho_of(t + 1), rho_of(t + 2)
        if re + ro >= 0:
            rho[t + 1], rho[t + 2] = re, ro
        t += 2
    max_t = t - 2
    if re > 0:
        rho[max_t + 1] = re
    u = 1
    while u <= max_t - 2:
        if rho[u + 1] + rho[u + 2] > rho[u - 1] + rho[u]:
            rho[u + 1] = rho[u + 2] = (rho[u - 1] + rho[u]) / 2.0
        u += 2
    tau = -1.0 + 2.0 * np.sum(rho[:max_t + 1]) + rho[max_t + 1]
    tau = max(tau, 1.0 / np.log10(M * n))
    return M * n / tau, t


def diagnostics(samples, burn=0):
    """Dict of [P] arrays: mean, sd, mcse_mean, ess, r_hat, max_lag (as chain_diagnostics)."""
    a = np.asarray(samples, dtype=np.float64)
    if a.ndim == 2:
        a = a[None]
    C, T, P = a.shape
    kept = a[:, burn:]
    Tp = T - burn
    n = Tp // 2
    assert n >= 4
    shift = kept[0, 0].copy()
    with np.errstate(invalid="ignore"):
        y = kept - shift
    seqs = np.stack([y[:, :n], y[:, Tp - n:]], axis=1).reshape(2 * C, n, P)
    M = 2 * C
    flat = kept.reshape(-1, P)
    with np.errstate(invalid="ignore"):
        out = dict(mean=shift + y.reshape(-1, P).mean(0), sd=y.reshape(-1, P).std(0, ddof=1))
    r_hat, ess = np.full(P, np.nan), np.full(P, np.nan)
    max_lag = np.zeros(P, dtype=np.int64)
    for j in range(P):
        x = seqs[:, :, j]
        if not np.all(np.isfinite(flat[:, j])):
            continue
        means = x.mean(1)
        W = x.var(1, ddof=1).mean()
        if W == 0:
            continue
        var_plus = (n - 1) / n * W + means.var(ddof=1)
        r_hat[j] = np.sqrt(var_plus / W)
        acov = autocov_fft(x - means[:, None]).mean(0)
        ess[j], max_lag[j] = ess_scan(acov, W, var_plus, n, M)
    out["r_hat"], out["ess"], out["max_lag"] = r_hat, ess, max_lag
    out["mcse_mean"] = out["sd"] / np.sqrt(ess)
    return {k: out[k] for k in ("mean", "sd", "mcse_mean", "ess", "r_hat", "max_lag")}


def ar1(rng, C, T, P, phi, loc=0.0, scale=1.0):
    """C chains of a stationary AR(1) process per column (innovation sd chosen for unit
    marginal variance), times `scale` plus `loc`."""
    z = rng.standard_normal((C, T, P))
    x = np.empty_like(z)
    x[:, 0] = z[:, 0]
    s = np.sqrt(1.0 - phi * phi)
    for t in range(1, T):
        x[:, t] = phi * x[:, t - 1] + s * z[:, t]
    return loc + scale * x
