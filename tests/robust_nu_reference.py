"""The Student-t Gibbs sweep with the degrees of freedom on a grid (bmc_robust_run_nu)
restated on the host.  TEST INFRASTRUCTURE ONLY: numpy from the definitions, nothing of the kernels'
text; the sweep is that of tests/robust_reference.py with nu read per sweep.

After steps 1-4 of robust_reference.chain at the nu in force (nu_init before the first sweep):

  5. T = sum_n (log lambda_n - lambda_n)
  6. l_g = h_g T + c_g, h_g = nu_g / 2, c_g = n (h_g log h_g - lgamma(h_g)) + log w_g in float64 (what
     the host hands the kernel; -inf where w_g = 0); p_g = exp(l_g - max l); P_g the running sums in
     grid order; the pick is #{g < G - 1 : P_g < u_t P_{G-1}}; a T that is not finite keeps the index.

``chain`` continues on the picks, or on a forced ``path`` (path[t] = the index in force after sweep
t), as the replay mode does.  ``nu_uniforms`` restates the STREAM_NU stream of the device-RNG mode on
top of tests/rng_reference.py.
"""
import math

import numpy as np

import rng_reference as R
import robust_reference as RR

LD = np.longdouble
STREAM_NU = 0x4E554446            # "NUDF"


def default_grid():
    """The default grid and prior of gibbs_sampler_robust(nu="estimate"), from its docstring:
    geomspace(1, 100, 64); Gamma(2, rate 0.1) density times nu_g; start nearest 4."""
    grid = np.geomspace(1.0, 100.0, 64)
    weight = grid * (grid * np.exp(-0.1 * grid))
    return grid, weight, int(np.argmin(np.abs(grid - 4.0)))


def log_prior_consts(grid, weight, n):
    """c_g in float64, term by term as written above."""
    out = np.empty(len(grid))
    for i, (nu, w) in enumerate(zip(grid, weight)):
        h = float(nu) / 2.0
        out[i] = float(n) * (h * math.log(h) - math.lgamma(h)) + math.log(w) if w > 0 else -np.inf
    return out


def nu_uniforms(seed, sweeps):
    """u_t of the device-RNG mode: the first uniform of Philox counter (t lo, t hi, STREAM_NU, 0)."""
    w = R.stream_words(seed, np.arange(sweeps, dtype=np.uint64), STREAM_NU)
    return R.u53_open0(w[..., 0], w[..., 1])


def pick(T, h, c, u, dtype):
    """(index, margin): margin = min_g |u P_{G-1} - P_g| / P_{G-1} over g < G - 1 (inf for G = 1)."""
    dt = dtype
    l = h.astype(dt) * dt(T) + c.astype(dt)
    p = np.exp(l - l.max())
    P = np.zeros(len(p), dtype=dt)
    run = dt(0)
    for g in range(len(p)):
        run = run + p[g]
        P[g] = run
    cut = dt(u) * P[-1]
    idx = int(np.count_nonzero(P[:-1] < cut))
    margin = float(np.min(np.abs(cut - P[:-1]) / P[-1])) if len(p) > 1 else np.inf
    return idx, margin


def chain(y, X, iters, prior, grid, weight, nu_init, xi, g, gl, u, burn=0, dtype=np.float64, path=None):
    """One chain.  xi (burn + iters, k), g (burn + iters,), u (burn + iters,); gl is (burn + iters, N)
    or a callable gl(t, grid index in force) -> (N,) for a free chain whose weight variates depend on
    the path.  Returns a dict: samples (iters, k + 1), weights (N,) the mean lambda over the kept
    sweeps, idx (iters,) the picks, tstat (iters,), margin (iters,) the picks' margins, path
    (burn + iters,) the index in force after every sweep."""
    dt = dtype
    b0, C0, nu0, s20 = prior
    grid = np.asarray(grid, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).astype(dt)
    X = np.asarray(X, dtype=np.float64).astype(dt)
    n, k = X.shape
    h = grid / 2.0
    c = log_prior_consts(grid, np.asarray(weight, dtype=np.float64), n)
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
    idx_out = np.zeros(iters, dtype=np.int64)
    t_out = np.zeros(iters, dtype=dt)
    m_out = np.full(iters, np.inf)
    went = np.zeros(burn + iters, dtype=np.int64)
    cur = int(nu_init)
    for t in range(burn + iters):
        nu = grid[cur]
        XtL = X.T * lam
        Q = XtL @ X / s2 + P + ridge
        rhs = Pb0 + XtL @ y / s2
        L = RR.cholesky(Q)
        z = np.zeros(k, dtype=dt)
        for i in range(k):
            z[i] = (rhs[i] - L[i, :i] @ z[:i]) / L[i, i]
        w = z + np.asarray(xi[t]).astype(dt)
        b = np.zeros(k, dtype=dt)
        for i in range(k - 1, -1, -1):
            b[i] = (w[i] - L[i + 1:, i] @ b[i + 1:]) / L[i, i]
        r = y - X @ b
        s2 = max(((dt(nu0) * dt(s20) + np.sum(lam * r * r)) / half) / dt(g[t]), dt(1e-6))
        glt = gl(t, cur) if callable(gl) else gl[t]
        lam = np.asarray(glt).astype(dt) / ((dt(nu) + r * r / s2) / half)
        T = np.sum(np.log(lam) - lam)
        new, margin = (pick(T, h, c, u[t], dt) if np.isfinite(T) else (cur, np.inf))
        if t >= burn:
            out[t - burn, :k] = b
            out[t - burn, k] = np.sqrt(s2)
            lsum += lam
            idx_out[t - burn], t_out[t - burn], m_out[t - burn] = new, T, margin
        cur = int(path[t]) if path is not None else new
        went[t] = cur
    return {"samples": out, "weights": lsum / dt(max(iters, 1)), "idx": idx_out, "tstat": t_out,
            "margin": m_out, "path": went}


def forced_path(n_grid, sweeps, chain_index, hold=4):
    """A path that changes value every ``hold`` sweeps and visits both ends of the grid: a fixed
    shuffle of the indices, rotated per chain."""
    order = np.array([(3 * i + chain_index) % n_grid for i in range(n_grid)]) if n_grid % 3 else \
        np.roll(np.arange(n_grid), chain_index)
    return order[(np.arange(sweeps) // hold) % n_grid].astype(np.int32)


def path_variates(n, k, sweeps, grid, nu_init, path, nu0, seed):
    """numpy variates of a forced-path replay: xi, g, gl at the shapes of the path, u."""
    rng = np.random.default_rng(seed)
    before = np.concatenate([[nu_init], path[:-1]])
    shape = (np.asarray(grid)[before] + 1.0) / 2.0
    return (rng.standard_normal((sweeps, k)), rng.gamma((nu0 + n) / 2, size=sweeps),
            rng.gamma(shape[:, None], size=(sweeps, n)), rng.random(sweeps))


def device_streams(seed, n, k, sweeps, grid, nu0):
    """The host-restated streams of a device-RNG chain: xi, g, the weight variates of every grid
    value (G, sweeps, n) with their accept margins (G, sweeps, n), u."""
    xi = R.normals(seed, sweeps * k).astype(np.float64).reshape(sweeps, k)
    g = R.gammas(seed, (nu0 + n) / 2, sweeps)[0]
    tabs = [RR.robust_gammas(seed, nu, n, sweeps) for nu in grid]
    return (xi, g, np.stack([t[0] for t in tabs]), np.stack([t[2] for t in tabs]),
            nu_uniforms(seed, sweeps))
