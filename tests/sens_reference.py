"""Dense numpy restatement of the power-scaling sensitivity (Kallioinen, Paananen, Buerkner &
Vehtari 2023), written from the estimator's definition (pybmc_amd/sensitivity.py states it), not
from the library.  Everything in ``dtype``: float64, or np.longdouble for the rounding floor.  The
Pareto fit and the tail length are those of psis_reference (r_eff = 1).

Per pooled draw: lp_beta, lp_sigma2, loglik (constants dropped; NaN for a draw with a non-finite
coefficient or without a finite sigma > 0).  Per (component, alpha): lw = (alpha - 1) lp, shifted,
smoothed as psis_reference.psis_row smooths it, normalised.  Per quantity column and weight vector:
the cumulative Jensen-Shannon distance and the weighted mean and sd."""
import numpy as np

from psis_reference import MIN_TAIL, gpdfit, tail_length

COMPONENTS = ("prior", "likelihood", "prior_beta", "prior_sigma2")
THRESHOLD = 0.05


def _cholesky(C, dtype):
    C = np.asarray(C, dtype=dtype)
    k = C.shape[0]
    L = np.zeros((k, k), dtype=dtype)
    for i in range(k):
        for j in range(i + 1):
            s = C[i, j] - (L[i, :j] * L[j, :j]).sum()
            if i == j:
                if not s > 0:
                    raise np.linalg.LinAlgError("C0 is not positive definite")
                L[i, i] = np.sqrt(s)
            else:
                L[i, j] = s / L[j, j]
    return L


def log_densities(A, y, theta, prior, dtype=np.float64):
    """(lp_beta, lp_sigma2, loglik), each [S]."""
    A = np.asarray(A, dtype=dtype)
    y = np.asarray(y, dtype=dtype)
    theta = np.asarray(theta, dtype=dtype)
    b0, C0, nu0, s20 = prior
    b0 = np.asarray(b0, dtype=dtype)
    nu0, s20 = dtype(nu0), dtype(s20)
    N, k = A.shape
    beta, sigma = theta[:, :k], theta[:, k]
    L = _cholesky(C0, dtype)
    with np.errstate(all="ignore"):
        d = beta - b0
        z = np.zeros_like(d)
        for i in range(k):                       # forward substitution, all draws at once
            z[:, i] = (d[:, i] - z[:, :i] @ L[i, :i]) / L[i, i]
        lp_beta = -(z * z).sum(axis=1) / 2
        s2 = sigma * sigma
        lp_sigma2 = -(nu0 / 2 + 1) * np.log(s2) - nu0 * s20 / (2 * s2)
        res = y[None, :] - beta @ A.T
        rss = (res * res).sum(axis=1)
        two_pi = 8 * np.arctan(dtype(1))
        loglik = -(dtype(N) / 2) * np.log(two_pi) - N * np.log(sigma) - rss / (2 * s2)
    bad = ~(np.isfinite(theta).all(axis=1) & (sigma > 0))
    for v in (lp_beta, lp_sigma2, loglik):
        v[bad] = np.nan
    return lp_beta, lp_sigma2, loglik


def component_vector(lp, name):
    lb, ls, ll = lp
    return {"prior": lb + ls, "likelihood": ll, "prior_beta": lb, "prior_sigma2": ls}[name]


def psis_weights(lp, alpha, dtype=np.float64):
    """(normalised weights [S], pareto_k) of lw = (alpha - 1) lp: psis_reference.psis_row's smoothing."""
    lp = np.asarray(lp, dtype=dtype)
    S = len(lp)
    lw = (dtype(alpha) - 1) * lp
    lw = lw - lw.max()
    M = tail_length(S)
    khat = dtype(np.inf)
    if M >= MIN_TAIL:
        order = np.argsort(lw, kind="stable")
        tail = order[S - M:]
        cutoff = lw[order[S - M - 1]]
        lt = lw[tail]
        if lt[0] != lt[-1]:
            with np.errstate(all="ignore"):
                ecut = np.exp(cutoff)
                k, sigma = gpdfit(np.exp(lt) - ecut, dtype)
                if np.isfinite(k):
                    khat = k
                    p = (np.arange(1, M + 1).astype(dtype) - dtype(0.5)) / M
                    if abs(k) < 1e-30:
                        q = -sigma * np.log1p(-p)
                    else:
                        q = sigma * np.expm1(-k * np.log1p(-p)) / k
                    lw = lw.copy()
                    lw[tail] = np.log(ecut + q)
        lw = np.minimum(lw, 0)
    w = np.exp(lw)
    return w / w.sum(), khat


def cjs_distance(x, w, dtype=np.float64, elementwise=True):
    """(cjs, weighted mean, weighted sd) of column x under the normalised weights w.
    elementwise: the two nearly cancelling terms of each direction are joined per element before
    they are summed (what float64 needs); False: the definition as it is written."""
    x = np.asarray(x, dtype=dtype)
    w = np.asarray(w, dtype=dtype)
    S = len(x)
    order = np.argsort(x, kind="stable")          # by (value, draw index)
    xs, ws = x[order], w[order]
    d = np.append(np.diff(xs), dtype(0))
    P = np.arange(1, S + 1).astype(dtype) / S
    Q = np.cumsum(ws)
    ln2 = np.log(dtype(2))
    IP, IQ = (P * d).sum(), (Q * d).sum()
    with np.errstate(all="ignore"):
        if elementwise:
            delta = Q - P
            tpq = d * ((-P * np.log1p(delta / (2 * P)) + delta / 2) / ln2)
            tq = np.where(Q == 0, P / 2, -Q * np.log1p(-delta / (2 * np.where(Q == 0, 1, Q))) - delta / 2)
            tqp = d * (tq / ln2)
            cpq, cqp = tpq.sum(), tqp.sum()
        else:
            m = (P + Q) / 2
            cpq = (d * P * np.log2(P / m)).sum() + (IQ - IP) / (2 * ln2)
            lq = np.where(Q == 0, 0, Q * np.log2(np.where(Q == 0, 1, Q) / m))
            cqp = (d * lq).sum() + (IP - IQ) / (2 * ln2)
    cpq, cqp = max(cpq, dtype(0)), max(cqp, dtype(0))
    den = IP + IQ
    cjs = np.sqrt((cpq + cqp) / den) if den != 0 else dtype(0)
    mean = (w * x).sum()
    sd = np.sqrt((w * (x - mean) ** 2).sum())
    return cjs, mean, sd


def quantities(theta, Vt, dtype=np.float64):
    """[S][k + 1 + M]: the coefficients, sigma and the model weights beta . Vt + 1 / M."""
    theta = np.asarray(theta, dtype=dtype)
    if Vt is None:
        return theta
    Vt = np.asarray(Vt, dtype=dtype)
    k = Vt.shape[0]
    with np.errstate(all="ignore"):
        om = theta[:, :k] @ Vt + dtype(1) / Vt.shape[1]
    return np.concatenate([theta, om], axis=1)


def sensitivity(A, y, theta, prior, Vt=None, alphas=(0.99, 1.01), components=("prior", "likelihood"),
                dtype=np.float64):
    """dict: lp (3, S); weights (c, a, S); pareto_k (c, a); mean, sd, cjs (c, a, Q); the flags.
    A component with a non-finite log density and a column with a non-finite value are NaN."""
    lp = log_densities(A, y, theta, prior, dtype)
    X = quantities(theta, Vt, dtype)
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


def psens(cjs_lo, cjs_hi, alpha_hi=1.01):
    return (cjs_lo + cjs_hi) / (2 * np.log2(alpha_hi))


def diagnose(p_prior, p_lik, threshold=THRESHOLD):
    if p_prior >= threshold and p_lik >= threshold:
        return "prior-data conflict"
    if p_prior >= threshold and p_lik < threshold:
        return "strong prior / weak likelihood"
    return "-"


# ---- cases --------------------------------------------------------------------------------------
def random_case(N, k, S, seed, n_models=0, dense_C0=True):
    """A well-conditioned synthetic fit: draws scattered about the least-squares point."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((N, k)) / np.sqrt(N)
    btrue = rng.standard_normal(k)
    y = A @ btrue + 0.3 * rng.standard_normal(N)
    theta = np.column_stack([btrue + 0.4 * rng.standard_normal((S, k)),
                             0.3 * np.exp(0.15 * rng.standard_normal(S))])
    G = rng.standard_normal((k, k))
    C0 = G @ G.T / k + np.eye(k) if dense_C0 else np.diag(1.0 + rng.random(k))
    prior = [0.1 * rng.standard_normal(k), C0, 1.0, 0.02]
    Vt = rng.standard_normal((k, n_models)) / np.sqrt(k) if n_models else None
    return A, y, theta, prior, Vt


def conflict_problem(seed=3, N=60, sigma=0.5):
    """One column, a tight prior far from the least-squares fit: (A, y, prior)."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((N, 1))
    y = 2.0 * A[:, 0] + sigma * rng.standard_normal(N)
    prior = [np.array([0.0]), np.array([[0.05]]), 1.0, 0.02]
    return A, y, prior


def conjugate_draws(A, y, prior, S, seed, sigma):
    """Exact draws of beta | y at fixed sigma (one column), sigma as the last column."""
    rng = np.random.default_rng(seed)
    b0, C0 = float(prior[0][0]), float(prior[1][0, 0])
    prec = 1.0 / C0 + float(A[:, 0] @ A[:, 0]) / sigma ** 2
    mean = (b0 / C0 + float(A[:, 0] @ y) / sigma ** 2) / prec
    beta = mean + rng.standard_normal(S) / np.sqrt(prec)
    return np.column_stack([beta, np.full(S, sigma)])
