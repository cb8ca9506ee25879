"""The Student-t (outlier-robust) Gibbs sweep and its weight-variate stream restated on the host.
TEST INFRASTRUCTURE ONLY: numpy from the definitions (DESIGN.md 4.12 and "Variate streams"), nothing
of the kernels' text.

Model: y_n | beta, sigma2, lambda_n ~ N(x_n . beta, sigma2 / lambda_n), lambda_n ~ Gamma(nu/2, rate
nu/2); priors beta ~ N(b0, C0) and the (nu0, sigma20) form for sigma2.  Start: lambda = 1, sigma2 =
max(mean r_ols^2, 1e-6).  Sweep t (P = inv(C0), L = diag(lambda)):

  1. Q = X'LX / sigma2 + P + 1e-6 I = L_c L_c';  beta = Q^-1 (P b0 + X'Ly / sigma2) + L_c^-T xi_t
  2. r = y - X beta;  sigma2 = max(((nu0 sigma20 + sum lambda_n r_n^2) / 2) / G_t, 1e-6)
  3. lambda_n = g_{t,n} / ((nu + r_n^2 / sigma2) / 2)
  4. record [beta, sqrt(sigma2)]; for t >= burn add lambda to the rows' running sums

``chain`` runs it in float64 or numpy.longdouble on explicit variates; ``robust_gammas`` restates
the STREAM_ROBUST stream of the device-RNG mode on top of tests/rng_reference.py.
"""
import numpy as np

import rng_reference as R

LD = np.longdouble
STREAM_ROBUST = 0x524F4253        # "ROBS"


def cholesky(Q):
    """Lower factor of a symmetric positive definite matrix in Q's own dtype, written out."""
    k = Q.shape[0]
    L = np.zeros_like(Q)
    for i in range(k):
        for j in range(i + 1):
            s = Q[i, j] - L[i, :j] @ L[j, :j]
            L[i, j] = np.sqrt(s) if i == j else s / L[j, j]
    return L


def chain(y, X, iters, prior, nu, xi, g, gl, burn=0, dtype=np.float64, freeze=False):
    """One chain on the variates xi (burn + iters, k), g (burn + iters,), gl (burn + iters, N).
    Returns (samples (iters, k + 1), mean lambda over the kept sweeps (N,)) in ``dtype``.  With
    ``freeze`` the weights stay 1: the Gaussian sampler on the same variates."""
    dt = dtype
    b0, C0, nu0, s20 = prior
    y = np.asarray(y, dtype=np.float64).astype(dt)
    X = np.asarray(X, dtype=np.float64).astype(dt)
    n, k = X.shape
    P = np.linalg.inv(np.asarray(C0, dtype=np.float64)).astype(dt)
    Pb0 = P @ np.asarray(b0, dtype=np.float64).astype(dt)
    X64 = X.astype(np.float64)
    bh = np.linalg.solve(X64.T @ X64, X64.T @ y.astype(np.float64)).astype(dt)
    s2 = max(np.mean((y - X @ bh) ** 2), dt(1e-6))
    lam = np.ones(n, dtype=dt)
    ridge = dt(1e-6) * np.eye(k, dtype=dt)
    half = dt(2)
    out = np.zeros((iters, k + 1), dtype=dt)
    lsum = np.zeros(n, dtype=dt)
    for t in range(burn + iters):
        XtL = X.T * lam
        Q = XtL @ X / s2 + P + ridge
        rhs = Pb0 + XtL @ y / s2
        L = cholesky(Q)
        z = np.zeros(k, dtype=dt)
        for i in range(k):
            z[i] = (rhs[i] - L[i, :i] @ z[:i]) / L[i, i]
        w = z + np.asarray(xi[t]).astype(dt)
        b = np.zeros(k, dtype=dt)
        for i in range(k - 1, -1, -1):
            b[i] = (w[i] - L[i + 1:, i] @ b[i + 1:]) / L[i, i]
        r = y - X @ b
        s2 = max(((dt(nu0) * dt(s20) + np.sum(lam * r * r)) / half) / dt(g[t]), dt(1e-6))
        if not freeze:
            lam = np.asarray(gl[t]).astype(dt) / ((dt(nu) + r * r / s2) / half)
        if t >= burn:
            out[t - burn, :k] = b
            out[t - burn, k] = np.sqrt(s2)
            lsum += lam
    return out, lsum / dt(max(iters, 1))


def robust_gammas(seed, nu, n_rows, sweeps, max_attempts=64):
    """g[t, n] ~ Gamma((nu + 1) / 2, 1) of the device-RNG mode: Marsaglia & Tsang as
    rng_reference.gammas, attempt m of (row n, sweep t) on the Philox counters
    (n, t lo32, STREAM_ROBUST, ((t >> 32) << 8) | 2m) and the same with | (2m + 1), keyed by seed.
    Returns (values (sweeps, n_rows) float64, attempts, margin): margin as rng_reference.gammas,
    the smallest distance of any accept / reject test an element went through from flipping."""
    a = (float(nu) + 1.0) / 2.0
    boost = a < 1.0
    aa = a + 1.0 if boost else a
    d = np.float64(aa) - np.float64(1.0) / np.float64(3.0)
    c = np.float64(1.0) / np.sqrt(np.float64(9.0) * d)
    dl, cl = LD(d), LD(c)
    total = sweeps * n_rows
    val = np.full(total, dl, dtype=LD)
    attempts = np.full(total, max_attempts, dtype=np.int64)
    margin = np.full(total, np.inf)
    inv_a = LD(np.float64(1.0) / np.float64(a))
    tt, nn = np.divmod(np.arange(total, dtype=np.uint64), np.uint64(n_rows))
    key = R._key(seed)
    todo = np.arange(total, dtype=np.int64)

    def words(idx, sub):
        ctr = np.empty((len(idx), 4), dtype=np.uint64)
        t = tt[idx]
        ctr[:, 0] = nn[idx]
        ctr[:, 1] = t & np.uint64(0xFFFFFFFF)
        ctr[:, 2] = STREAM_ROBUST
        ctr[:, 3] = ((t >> np.uint64(32)) << np.uint64(8)) | np.uint64(sub)
        return R.philox4x32_10(ctr, key)

    for m in range(max_attempts):
        if len(todo) == 0:
            break
        x, _, _ = R.box_muller(*R.pair_uniforms(words(todo, 2 * m)))
        u, ub = R.pair_uniforms(words(todo, 2 * m + 1))
        lin = LD(1) + cl * x
        mg = np.abs(lin)
        pos = lin > 0
        v = np.where(pos, lin, LD(1)) ** 3
        x2 = x * x
        squeeze = LD(1) - LD(0.0331) * x2 * x2
        rhs = LD(0.5) * x2 + dl * (LD(1) - v + np.log(v))
        ul = u.astype(LD)
        lu = np.log(ul)
        tests = np.minimum(np.abs(ul - squeeze), np.abs(lu - rhs))
        mg = np.where(pos, np.minimum(mg, tests), mg)
        margin[todo] = np.minimum(margin[todo], mg.astype(np.float64))
        ok = pos & ((ul < squeeze) | (lu < rhs))
        res = dl * v
        if boost:
            res = res * ub.astype(LD) ** inv_a
        val[todo[ok]] = res[ok]
        attempts[todo[ok]] = m + 1
        todo = todo[~ok]
    shape = (sweeps, n_rows)
    return val.astype(np.float64).reshape(shape), attempts.reshape(shape), margin.reshape(shape)


def planted_problem(n, k, frac, seed):
    """The planted-outlier problem of the issue: orthonormal X (leading left singular vectors of a
    centred random matrix), y = X beta* + 0.1 z, a share ``frac`` of the rows shifted by 8 .. 16
    sigma in a random direction.  Returns (y, X, prior, beta*, planted row indices)."""
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((n, k + 1))
    F -= F.mean(1, keepdims=True)
    U, S, _ = np.linalg.svd(F, full_matrices=False)
    X, S = np.ascontiguousarray(U[:, :k]), S[:k]
    bs = rng.standard_normal(k) * 3
    sig = 0.1
    y = X @ bs + sig * rng.standard_normal(n)
    m = int(frac * n)
    idx = rng.choice(n, m, replace=False)
    y[idx] += 8.0 * sig * np.where(rng.random(m) < 0.5, -1, 1) * (1 + rng.random(m))
    prior = (np.zeros(k), np.diag(S ** 2), 1.0, 0.02)
    return y, X, prior, bs, np.sort(idx)


def host_variates(n, k, sweeps, nu, nu0, seed):
    """numpy variates for a replay run: xi (sweeps, k), g (sweeps,), gl (sweeps, n)."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((sweeps, k)), rng.gamma((nu0 + n) / 2, size=sweeps),
            rng.gamma((nu + 1) / 2, size=(sweeps, n)))
