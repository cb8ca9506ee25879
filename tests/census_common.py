"""Problems, oracle chains and planner access of the kernel census tests (test_kernel_census.py on
the CPU, test_kernel_census_gpu.py on the GPU).  tests/kernel_census.txt holds one line per compiled
loop kernel: "name | recipe" or "name | unreached" (tests/launch_plan_check.cpp, mode census).

Perturbed oracles.  A loop kernel computes two things per iteration: the draw from its variates and
the residual sum of squares over its row panels.  The sensitivity checks therefore perturb exactly
those inside the otherwise unchanged oracle loop: rss without the last row, rss with the last
column of X taken as zero, and the gamma variates of another chain (zeroing the column in the
problem itself would make X'X singular, which is a different problem, not a wrong kernel)."""
import os
import subprocess

import numpy as np

from oracle import bmc_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "kernel_census.txt")
T_GIBBS = 130            # crosses the 64-row output staging block twice and leaves a remainder
BURN_SIMPLEX, T_SIMPLEX = 70, 130
N_STREAMS = 5            # distinct oracle chains per problem at most (slot colouring below)
F64_BAR = 1e-9           # the project's replay bar, times max(1, |ref|.max())
F32_SUMMARY_BAR = 1e-5   # test_t2_float32_storage's bar on posterior_summary
F32_CHAIN_CAP = 1e-5
MARGIN = 1e-6            # smallest accept/reject decision margin a simplex problem may have
SIMPLEX_SEED = 1         # what the seed search of simplex_case finds for every problem of the census
                         # (smallest margin over them 1.8e-3); the GPU test asserts it, so that a
                         # change of data or recipes that moves a seed is seen
STEPSIZES = (0.3, 0.1, 0.03, 0.01, 0.003, 0.001, 0.0003, 0.0001)


def build_planner(tmpdir):
    exe = os.path.join(str(tmpdir), "launch_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-o", exe,
                    os.path.join(HERE, "launch_plan_check.cpp")], check=True)
    return exe


def parse_recipe(text):
    """'gibbs n=.. k=.. ...' -> dict (sampler + integer fields), 'unreached' -> None."""
    if text == "unreached":
        return None
    parts = text.split()
    r = {"sampler": parts[0]}
    r.update((a, int(b)) for a, b in (p.split("=") for p in parts[1:]))
    return r


def read_table(path=TABLE):
    """[(kernel name, recipe dict or None)] in table order."""
    with open(path) as f:
        rows = [line.rstrip("\n").split(" | ", 1) for line in f if line.strip()]
    return [(name, parse_recipe(rec)) for name, rec in rows]


def parse_launches(text):
    """'kernel@c0+n:cpp;...' -> [(kernel, c0, n, cpp)]."""
    out = []
    for item in text.strip().split(";"):
        name, rest = item.rsplit("@", 1)
        c0, rest = rest.split("+")
        n, cpp = rest.split(":")
        out.append((name, int(c0), int(n), int(cpp)))
    return out


def replan(exe, path=TABLE):
    """{kernel name: None | (launches as planned with the recipe's pack answer, with the other)}."""
    res = subprocess.run([exe, "replan", path], check=True, capture_output=True, text=True).stdout
    out = {}
    for line in res.splitlines():
        cols = line.split(" | ")
        out[cols[0]] = None if cols[1] == "unreached" else (parse_launches(cols[1]), parse_launches(cols[2]))
    return out


def problem_key(r):
    return (r["sampler"], r["n"], r["k"], r["f32"], r.get("ow", 0))


# ---- data ---------------------------------------------------------------------------------------
def gibbs_problem(n, k, f32):
    """Columns of unequal scale (1 .. 1/4), mixed so that X is far from orthonormal, noise sd 0.1,
    and an outlier in the last row.  With f32 storage the problem IS its f32 rounding (float64
    arrays holding f32 values), as the device stores it."""
    rng = np.random.default_rng([n, k])
    mix = np.eye(k) + 0.35 * rng.standard_normal((k, k)) / np.sqrt(k)
    X = (rng.standard_normal((n, k)) @ mix) * np.geomspace(1.0, 0.25, k)[None, :]
    b = np.where(np.arange(k) % 2 == 0, 0.8, -0.6) * (1.0 - 0.3 * (np.arange(k) % 3) / 2)
    y = X @ b + 0.1 * rng.standard_normal(n)
    y[n - 1] += 10.0
    if f32:
        X, y = X.astype(np.float32).astype(float), y.astype(np.float32).astype(float)
    prior = (np.zeros(k), np.eye(k) * 10.0, 1.0, 0.02)
    return y, X, prior


def simplex_problem(n, k, f32, ow):
    """Vt_hat, S_hat and X = U_hat from an SVD of a centred synthetic model matrix (n_models <= 64
    where the recipe needs the one-wave form, > 64 where it needs the workgroup form), y with the
    outlier in the last row."""
    km = k + 2 if ow else max(65, k + 2)
    rng = np.random.default_rng([n, k, 1])
    A = rng.standard_normal((n, km)) * np.geomspace(1.0, 0.25, km)[None, :]
    truth = A @ np.full(km, 1.0 / km) + 0.05 * rng.standard_normal(n)
    Ac = A - A.mean(1, keepdims=True)
    U, S, Vt = np.linalg.svd(Ac, full_matrices=False)
    X = np.ascontiguousarray(U[:, :k])
    S_hat = S[:k]
    Vt_hat = Vt[:k] / S_hat[:, None]
    y = truth - A.mean(1)
    y[n - 1] += 10.0
    if f32:
        X, y = X.astype(np.float32).astype(float), y.astype(np.float32).astype(float)
    return y, X, Vt_hat, S_hat


# ---- Gibbs oracle chains ------------------------------------------------------------------------
def gibbs_chain(y, X, prior, Z, G, rss_fn=None):
    """O.gibbs_replay with the residual sum of squares replaceable (None: O.residual_rss, and the
    chain is O.gibbs_replay's bit for bit).  Returns (chain, sigma2 trace)."""
    st = O.chain_setup(y, X, prior)
    s2 = st["sigma2_init"]
    T, K = Z.shape
    out, trace = np.empty((T, K + 1)), np.empty(T + 1)
    trace[0] = s2
    for t in range(T):
        mean, cov = O.conditional_moments(st, y, X, s2)
        beta = O.mvn_draw_svd(mean, cov, Z[t])
        rss = O.residual_rss(y, X, beta) if rss_fn is None else rss_fn(beta)
        s2 = O.sigma2_draw(st, rss, G[t])
        out[t, :K] = beta
        out[t, K] = np.sqrt(s2)
        trace[t + 1] = s2
    return out, trace


def gibbs_streams(y, X, prior, n_streams, T=T_GIBBS):
    n, k = X.shape
    shape = (prior[2] + n) / 2.0
    return [O.reference_streams(1000 + 2 * s, 1001 + 2 * s, T, k, shape) for s in range(n_streams)]


def oracle_basis(y, X, prior):
    """W of DESIGN.md's rotated draw from the oracle's own quantities: B = P + 1e-6 I = L L',
    L^-1 X'X L^-T = Q diag(lam) Q', W = L^-T Q."""
    st = O.chain_setup(y, X, prior)
    L = np.linalg.cholesky(st["P"] + O.RIDGE * np.eye(X.shape[1]))
    Li = np.linalg.inv(L)
    lam, Q = np.linalg.eigh(Li @ st["XtX"] @ Li.T)
    return Li.T @ Q


def f32_rotation_error(y, X, prior, Z, G):
    """How far the oracle chain of an f32 problem moves when the residual is computed from the
    rotated panels X W rounded to f32 (what the device stores besides X and y), relative to
    max(1, |chain|.max())."""
    ref, _ = gibbs_chain(y, X, prior, Z, G)
    W = oracle_basis(y, X, prior)
    Xr = (X @ W).astype(np.float32).astype(float)
    Winv = np.linalg.inv(W)
    alt, _ = gibbs_chain(y, X, prior, Z, G, lambda beta: np.sum((y - Xr @ (Winv @ beta)) ** 2))
    return np.abs(alt - ref).max() / max(1.0, np.abs(ref).max())


def gibbs_sensitivity(y, X, prior, streams, ref):
    """Relative distance (over max(1, |ref|.max())) of the three perturbed oracles from chain 0."""
    (Z, G), (_, G1) = streams[0], streams[1 % len(streams)]
    if len(streams) == 1:
        G1 = O.reference_streams(999, 998, len(G), X.shape[1], (prior[2] + len(y)) / 2.0)[1]
    Xz = X.copy()
    Xz[:, -1] = 0.0
    scale = max(1.0, np.abs(ref).max())
    alts = {"last row dropped": gibbs_chain(y, X, prior, Z, G, lambda b: O.residual_rss(y[:-1], X[:-1], b))[0],
            "last column zero": gibbs_chain(y, X, prior, Z, G, lambda b: O.residual_rss(y, Xz, b))[0],
            "gamma stream of the next chain": gibbs_chain(y, X, prior, Z, G1)[0]}
    return {what: np.abs(alt - ref).max() / scale for what, alt in alts.items()}


def slot_groups(launches):
    """The chains that must replay pairwise different streams: the first, one middle and the last
    chain of every launch and of every bundle (launches: [(kernel, c0, chains, cpp)])."""
    groups = []
    for _, c0, nc, cpp in launches:
        spans = [(c0, c0 + nc)] + ([(b0, b0 + cpp) for b0 in range(c0, c0 + nc, cpp)] if cpp > 1 else [])
        groups += [sorted({a, (a + b - 1) // 2, b - 1}) for a, b in spans]
    return groups


def assert_separated(colour, launches):
    for group in slot_groups(launches):
        assert len({colour[c] for c in group}) == len(group), (group, [colour[c] for c in group])


def colour_slots(launches, n_colours=N_STREAMS, also=()):
    """Stream index per chain such that every group of slot_groups(launches) gets pairwise
    different streams (greedy colouring: a chain has at most four such neighbours, five colours
    suffice).  also: the launches of the plan with the other pack answer, separated as well when
    the colours reach (the caller asserts the separation for the plan the device took)."""
    if also and list(also) != list(launches):
        try:
            return colour_slots(list(launches) + list(also), n_colours)
        except StopIteration:
            pass
    n = max(l[1] + l[2] for l in launches)
    neigh = [set() for _ in range(n)]
    for group in slot_groups(launches):
        for c in group:
            neigh[c].update(j for j in group if j != c)
    colour = [-1] * n
    for c in range(n):
        used = {colour[j] for j in neigh[c] if colour[j] >= 0}
        colour[c] = next(x % n_colours for x in range(c, c + n_colours) if x % n_colours not in used)
    assert_separated(colour, launches)
    return colour


def plan_launches(exe, tmpdir, n, k, f32, chains, res=0, cpp=0, G=0, W=0, ppw=0, cu=0):
    """The CPU planner's launches for one Gibbs run, under both pack answers: ([..], [..])."""
    path = os.path.join(str(tmpdir), "recipe.txt")
    with open(path, "w") as f:
        f.write(f"run | gibbs n={n} k={k} f32={int(f32)} chains={chains} cu={cu} G={G} W={W} res={res} "
                f"ppw={ppw} cpp={cpp} pack=1 ow=0\n")
    return replan(exe, path)["run"]


# ---- simplex oracle -----------------------------------------------------------------------------
def simplex_streams(n, k, seed, tt):
    rs = np.random.RandomState(seed)
    Z = rs.standard_normal((tt, k))
    U = rs.uniform(size=tt)
    G = np.random.Generator(np.random.PCG64(seed + 1)).standard_gamma((1.0 + n) / 2, size=tt)
    return Z, U, G


def simplex_chain(y, X, Vt_hat, S_hat, stepsize, Z, U, G, burn=BURN_SIMPLEX, T=T_SIMPLEX, rss_fn=None):
    """O.simplex_replay with the diagonal proposal map (test_device_generator_distribution) and
    prior (1.0, 0.02); with rss_fn the same loop with the residual sum of squares replaced.
    Returns (chain, accepted in the sampling phase, uniforms used, accepted over burn + T,
    smallest decision margin |log u - log ratio|)."""
    step = S_hat * stepsize
    nm = Vt_hat.shape[1]
    n = len(y)
    rss = (lambda b: np.sum((y - X.dot(b)) ** 2)) if rss_fn is None else rss_fn
    b_cur = np.zeros(X.shape[1])
    ll_cur = -rss(b_cur)
    s2 = -ll_cur / n
    out, acc, acc_all, iu, margin = [], 0, 0, 0, np.inf
    for t in range(burn + T):
        b_prop = b_cur + step * Z[t]
        if not np.any(np.dot(b_prop, Vt_hat) + 1.0 / nm < 0):
            ll_prop = -rss(b_prop)
            log_ratio = (ll_prop - ll_cur) / s2
            u = U[iu]
            iu += 1
            margin = min(margin, abs(np.log(u) - min(0.0, log_ratio)))
            if u < min(1, np.exp(log_ratio)):
                b_cur, ll_cur = b_prop, ll_prop
                acc_all += 1
                acc += t >= burn
        s2 = 1 / (G[t] * (1 / ((1.0 * 0.02 - ll_cur) / 2.0)))
        if t >= burn:
            out.append(np.append(b_cur, np.sqrt(s2)))
    chain = np.array(out)
    if rss_fn is None:   # the loop above must BE the oracle
        real = O.mvn_draw_svd
        O.mvn_draw_svd = lambda mean, cov, z: mean + step * z
        try:
            ref, acc_ref, used_ref = O.simplex_replay(y, X, Vt_hat, S_hat, T, [1.0, 0.02], burn, stepsize, Z, U, G)
        finally:
            O.mvn_draw_svd = real
        assert np.array_equal(ref, chain) and acc_ref == acc and used_ref == iu
    return chain, acc, iu, acc_all, margin


def simplex_case(n, k, f32, ow):
    """Data, the first stepsize whose oracle chain both accepts and rejects (acceptances over
    burn + T strictly between 1/8 and 7/8 of it), and the first stream seed whose smallest decision
    margin is at least MARGIN.  f32 storage rounds X and y only (the sampler reads the un-rotated
    panels), so the margin and the bars are those of f64."""
    y, X, Vt_hat, S_hat = simplex_problem(n, k, f32, ow)
    tt = BURN_SIMPLEX + T_SIMPLEX
    for seed in range(1, 20):
        Z, U, G = simplex_streams(n, k, seed, tt)
        for stepsize in STEPSIZES:
            chain, acc, used, acc_all, margin = simplex_chain(y, X, Vt_hat, S_hat, stepsize, Z, U, G)
            if tt / 8 < acc_all < 7 * tt / 8:
                break
        else:
            raise AssertionError("no stepsize both accepts and rejects")
        if margin >= MARGIN:
            return dict(y=y, X=X, Vt_hat=Vt_hat, S_hat=S_hat, stepsize=stepsize, seed=seed, Z=Z, U=U, G=G,
                        chain=chain, acc=acc, used=used, acc_all=acc_all, margin=margin)
    raise AssertionError("no stream seed with a decision margin >= %g" % MARGIN)


def simplex_sensitivity(c):
    y, X = c["y"], c["X"]
    Xz = X.copy()
    Xz[:, -1] = 0.0
    args = (y, X, c["Vt_hat"], c["S_hat"], c["stepsize"], c["Z"], c["U"])
    G1 = simplex_streams(len(y), X.shape[1], c["seed"] + 100, len(c["G"]))[2]
    ref = c["chain"]
    scale = max(1.0, np.abs(ref).max())
    alts = {"last row dropped": simplex_chain(*args, c["G"], rss_fn=lambda b: np.sum((y[:-1] - X[:-1].dot(b)) ** 2))[0],
            "last column zero": simplex_chain(*args, c["G"], rss_fn=lambda b: np.sum((y - Xz.dot(b)) ** 2))[0],
            "gamma stream of another chain": simplex_chain(*args, G1, rss_fn=lambda b: np.sum((y - X.dot(b)) ** 2))[0]}
    return {what: np.abs(alt - ref).max() / scale for what, alt in alts.items()}
