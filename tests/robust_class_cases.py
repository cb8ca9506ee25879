"""Problems, variates and recorded reference deviations of the Student-t sampler's launch-class tests
(test_robust_classes_host.py on the CPU, test_robust_classes_gpu.py on the GPU): one shape per slab
edge and kernel width, a dense prior, burn-in, grids of 2 .. 64 values, poisoned variates for the
stopped-chain contract and device-RNG runs below shape 1.  TEST INFRASTRUCTURE ONLY.

REF_DEV holds, per case, the deviation of the FLOAT64 numpy reference from the long-double one on the
same variates (the max over the chains): samples relative to each column's scale, row weights relative
to the largest and, for the nu-grid cases, T_t relative to n.  ``bars`` turns an entry into the GPU
tests' bars, the rule of test_robust_gpu.py: BAR_FACTOR x the deviation, taken no smaller than 2^-52
(on the tiny shapes the two references can agree to the last bit, and one ulp of the scale is the
least a float64 result can be held to).  test_robust_classes_host.py recomputes every entry.
"""
import functools

import numpy as np

import rng_reference as R
import robust_cases as RC
import robust_nu_cases as NC
import robust_nu_reference as NR
import robust_reference as RR

LD = np.longdouble
BAR_FACTOR = 1000.0
DEV_FLOOR = 2.0 ** -52

# (N, k): the slab and width classes
#   1 x 1    wave 0 a partial k-step, waves 1-3 empty; KC = 4; the start value on the 1e-6 floor
#   2 x 1    the same slabs, a residual that is not zero
#   4 x 2    wave 0 exactly one k-step
#   5 x 4    the first row of wave 1; KC = 4 full
#   16 x 8   every wave one full k-step; KC = 8 full
#   17 x 9   rows_per_wave 8, wave 3 empty again; KC = 16 with seven identity rows
#   40 x 31  KC = 32 with one identity row, the second MFMA tile nearly full
#   256 x 3  one row per lane in phases B and L
SHAPES = ((1, 1), (2, 1), (4, 2), (5, 4), (16, 8), (17, 9), (40, 31), (256, 3))
COL_MAJOR = ((5, 4), (17, 9))
NU_SHAPES = ((5, 4), (16, 8), (17, 9), (40, 31))
CHAINS = 3
NU = 4.0
BURN, ITERS = 20, 100

# section C: the sweep of each chain whose G_t is 1e300 (the last one leaves one row behind it)
FLOOR_SHAPE = (17, 9)
FLOOR_SWEEPS = (30, 57, 118)
# section D
STOP_SHAPE = (17, 9)
STOP_BURN, STOP_ITERS, STOP_T0, STOP_EARLY_T0 = 10, 40, 30, 4
POISONS = ("inf", "negative", "nan")
# section E
GRID_SHAPE = (5, 4)
GRID_BURN, GRID_ITERS = 10, 50
GRID_SIZES = (2, 8, 9, 64)
ZERO_WEIGHT = (0, 4, 8)                 # of the grid of 9
EDGE_SWEEPS = (GRID_BURN + 5, GRID_BURN + 11)        # chain 0: u = 2^-53, then 1 - 2^-53
NONFINITE_CHAIN, NONFINITE_SWEEP = 1, GRID_BURN + 7
# section B, device mode with burn-in on RC.device_problem(); section F, device RNG below shape 1.
# test_robust_classes_host.py proves the margins of every seed.
BURN_DEVICE_SEEDS = (20261, 20262)
BURN_DEVICE_BURN, BURN_DEVICE_ITERS = 37, 50
LOW_N, LOW_K, LOW_NU, LOW_T = 17, 2, 0.5, 60
LOW_SEEDS = (40101, 40102)
LOW_GRID = np.array([0.5, 1.0, 2.0, 4.0, 8.0])
LOW_WEIGHT = np.ones(5)
LOW_INIT = 0
LOW_NU_SEEDS = (40201, 40202)

# measured on the CPU (numpy with OpenBLAS, x87 long double); "C" is large because the sweeps after a
# floored sigma2 = 1e-6 work on a Q of order 1e7
REF_DEV = {
    "1x1": (1.833e-16, 2.801e-16), "2x1": (1.978e-16, 2.396e-16), "4x2": (5.341e-16, 5.721e-16),
    "5x4": (7.777e-16, 6.313e-16), "16x8": (2.933e-15, 6.758e-16), "17x9": (4.154e-15, 5.565e-16),
    "40x31": (8.157e-15, 7.294e-16), "256x3": (1.721e-15, 7.078e-16),
    "C": (7.369e-13, 6.518e-14),
    "A-5x4": (5.076e-16, 8.553e-16, 5.013e-16), "A-16x8": (4.202e-15, 5.691e-16, 1.376e-15),
    "A-17x9": (7.041e-15, 6.791e-16, 2.745e-15), "A-40x31": (9.541e-15, 8.273e-16, 2.093e-15),
    "E-G2": (4.580e-16, 7.550e-16, 7.711e-16), "E-G8": (4.088e-15, 4.825e-16, 2.101e-15),
    "E-G9": (3.268e-16, 2.378e-16, 3.098e-16), "E-G64": (4.300e-16, 6.070e-16, 3.220e-16),
    "E-zero": (5.349e-16, 2.667e-16, 3.235e-16), "E-edges": (3.455e-15, 3.025e-16, 1.357e-15),
    "E-nonfinite": (1.727e-15, 3.423e-16, 6.540e-16),
    "F-fixed": (1.904e-15, 2.913e-15), "F-nu": (9.665e-16, 4.610e-16, 2.202e-15),
}


def bars(name):
    """The GPU bars of a case: BAR_FACTOR x max(recorded deviation, 2^-52) per quantity."""
    return tuple(BAR_FACTOR * max(d, DEV_FLOOR) for d in REF_DEV[name])


# ---- problems ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problem(n, k):
    """y and X of robust_cases.problem's dense recipe under a dense prior: C0 = G G' / k + I with G
    standard normal, b0 = 0.3 z.  The precision has off-diagonals and P b0 != 0."""
    y, X, prior = RC.problem(n, k)
    rng = np.random.default_rng(770000 + 1000 * n + k)
    G = rng.standard_normal((k, k))
    return y, X, (0.3 * rng.standard_normal(k), G @ G.T / k + np.eye(k), prior[2], prior[3])


def as_passed(n, k, X):
    """X in the layout the GPU tests hand to bmc_set_problem for this shape."""
    return np.asfortranarray(X) if (n, k) in COL_MAJOR else X


def low_problem():
    """The 17 x 2 problem of section F."""
    rng = np.random.default_rng(17002)
    X = rng.standard_normal((LOW_N, LOW_K)) + 0.3 * rng.standard_normal((LOW_N, 1))
    y = X @ np.array([1.0, -0.5]) + 0.3 * rng.standard_normal(LOW_N)
    y[[3, 11]] += 4.0
    return y, X, (np.array([0.2, -0.1]), np.array([[1.5, 0.4], [0.4, 2.0]]), 1.0, 0.02)


def start_sigma2(n, k, dtype=LD):
    """mean r_ols^2 of a problem, before the 1e-6 floor, as the reference computes it."""
    y, X, _ = problem(n, k)
    bh = np.linalg.solve(X.T @ X, X.T @ y).astype(dtype)
    return np.mean((y.astype(dtype) - X.astype(dtype) @ bh) ** 2)


# ---- fixed nu, replay -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixed_inputs(n, k, burn=BURN, iters=ITERS):
    """xi (C, T, k), g (C, T), gl (C, T, N), T = burn + iters: three chains, different variates.
    Shared and read-only: ``poisoned`` and ``floor_inputs`` copy."""
    nu0 = problem(n, k)[2][2]
    parts = [RR.host_variates(n, k, burn + iters, NU, nu0, seed=611953 * n + 89 * k + 7 * burn + c)
             for c in range(CHAINS)]
    out = tuple(np.stack([p[i] for p in parts]) for i in range(3))
    for a in out:
        a.setflags(write=False)
    return out


def run_fixed(n, k, xi, g, gl, burn, iters, dtype=LD, nu=NU):
    """(samples (C, iters, k + 1), weights (C, N)) of RR.chain per chain."""
    y, X, prior = problem(n, k)
    with np.errstate(all="ignore"):
        runs = [RR.chain(y, X, iters, prior, nu, xi[c], g[c], gl[c], burn=burn, dtype=dtype)
                for c in range(len(xi))]
    return np.stack([r[0] for r in runs]), np.stack([r[1] for r in runs])


@functools.lru_cache(maxsize=None)
def fixed_reference(n, k, dtype=LD):
    return run_fixed(n, k, *fixed_inputs(n, k), BURN, ITERS, dtype)


@functools.lru_cache(maxsize=None)
def floor_inputs():
    """Section C: the variates of FLOOR_SHAPE with G_t = 1e300 at one kept sweep per chain."""
    xi, g, gl = fixed_inputs(*FLOOR_SHAPE)
    g = g.copy()
    for c, t0 in enumerate(FLOOR_SWEEPS):
        g[c, t0] = 1e300
    return xi, g, gl


@functools.lru_cache(maxsize=None)
def floor_reference(dtype=LD):
    return run_fixed(*FLOOR_SHAPE, *floor_inputs(), BURN, ITERS, dtype)


def poisoned(kind, chains=(1,), t0=STOP_T0):
    """Section D: copies of the STOP_SHAPE variates with sweep t0 of ``chains`` poisoned."""
    xi, g, gl = (a.copy() for a in fixed_inputs(*STOP_SHAPE, STOP_BURN, STOP_ITERS))
    for c in chains:
        if kind == "inf":
            gl[c, t0, 3] = np.inf           # the next sweep's first pivot is +inf
        elif kind == "negative":
            gl[c, t0, :] = -50.0            # ... is negative
        elif kind == "nan":
            xi[c, t0, 2] = np.nan           # ... is NaN
        else:
            raise ValueError(kind)
    return xi, g, gl


def pivots_after(n, k, xi, g, gl, t0):
    """The long-double Cholesky pivots of sweep t0 + 1 of one chain, from the state RR.chain leaves
    after sweep t0 (its one kept row and that sweep's weights): Q_ii - sum_j L_ij^2 in order, up to
    and including the first that is not positive."""
    y, X, prior = problem(n, k)
    with np.errstate(all="ignore"):
        row, lam = RR.chain(y, X, 1, prior, NU, xi, g, gl, burn=t0, dtype=LD)
    s2 = row[0, k] ** 2
    Xl = X.astype(LD)
    Q = (Xl.T * lam) @ Xl / s2 + np.linalg.inv(prior[1]).astype(LD) + LD(1e-6) * np.eye(k, dtype=LD)
    L = np.zeros_like(Q)
    out = []
    with np.errstate(all="ignore"):
        for i in range(k):
            for j in range(i):
                L[i, j] = (Q[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
            out.append(Q[i, i] - L[i, :i] @ L[i, :i])
            if not out[-1] > 0:
                break
            L[i, i] = np.sqrt(out[-1])
    return out


# ---- nu on a grid, replay on forced paths -----------------------------------------------------------
NU_CASES = tuple(f"A-{n}x{k}" for n, k in NU_SHAPES) + tuple(f"E-G{G}" for G in GRID_SIZES) + \
    ("E-zero", "E-edges", "E-nonfinite")


def _grid(G):
    return np.geomspace(1.2, 60.0, G), 1.0 + 0.5 * (np.arange(G) % 3)


@functools.lru_cache(maxsize=None)
def nu_case(name):
    """A dict: n, k, grid, weight, init, burn, iters, paths (C, T) int32, xi, g, gl, u."""
    allowed, hold = None, 4
    if name.startswith("A-"):
        n, k = (int(v) for v in name[2:].split("x"))
        grid, weight, init, burn, iters = NC.GRID, NC.WEIGHT, NC.NU_INIT, BURN, ITERS
    elif name == "D":
        (n, k), burn, iters = STOP_SHAPE, STOP_BURN, STOP_ITERS
        grid, weight, init = NC.GRID, NC.WEIGHT, NC.NU_INIT
    else:
        (n, k), burn, iters = GRID_SHAPE, GRID_BURN, GRID_ITERS
        G = int(name[3:]) if name.startswith("E-G") else 9
        grid, weight = _grid(G)
        init = min(1, G - 1)
        if name == "E-zero":
            weight = weight.copy()
            weight[list(ZERO_WEIGHT)] = 0.0
            allowed = np.flatnonzero(weight > 0)
        hold = 1 if G == 64 else 4              # 60 sweeps reach both ends of the 64
    T = burn + iters
    allowed = np.arange(len(grid)) if allowed is None else allowed
    paths = np.stack([allowed[NR.forced_path(len(allowed), T, c, hold)] for c in range(CHAINS)]).astype(np.int32)
    nu0 = problem(n, k)[2][2]
    seed = 1299709 * n + 97 * k + 1009 * len(grid) + 10 * sum(map(ord, name))
    parts = [NR.path_variates(n, k, T, grid, init, paths[c], nu0, seed=seed + c) for c in range(CHAINS)]
    xi, g, gl, u = (np.stack([p[i] for p in parts]) for i in range(4))
    if name == "E-edges":
        u[0, EDGE_SWEEPS[0]] = 2.0 ** -53
        u[0, EDGE_SWEEPS[1]] = 1.0 - 2.0 ** -53
    if name == "E-nonfinite":
        gl[NONFINITE_CHAIN, NONFINITE_SWEEP, 0] = 0.0       # lambda = 0: T_t = -inf
    for a in (paths, xi, g, gl, u):
        a.setflags(write=False)
    return dict(n=n, k=k, grid=grid, weight=weight, init=init, burn=burn, iters=iters, paths=paths,
                xi=xi, g=g, gl=gl, u=u)


def run_nu(case, xi, g, gl, u, dtype=LD):
    """NR.chain per chain on the case's forced paths: a list of its dicts."""
    y, X, prior = problem(case["n"], case["k"])
    with np.errstate(all="ignore"):
        return [NR.chain(y, X, case["iters"], prior, case["grid"], case["weight"], case["init"], xi[c], g[c],
                         gl[c], u[c], burn=case["burn"], dtype=dtype, path=case["paths"][c])
                for c in range(len(xi))]


@functools.lru_cache(maxsize=None)
def nu_reference(name, dtype=LD):
    c = nu_case(name)
    return run_nu(c, c["xi"], c["g"], c["gl"], c["u"], dtype)


def nu_poisoned(kind, chains=(1,), t0=STOP_T0):
    """Section D on the grid: copies of case "D"'s variates with sweep t0 of ``chains`` poisoned."""
    c = nu_case("D")
    xi, g, gl = c["xi"].copy(), c["g"].copy(), c["gl"].copy()
    for ch in chains:
        if kind == "inf":
            gl[ch, t0, 3] = np.inf
        elif kind == "negative":
            gl[ch, t0, :] = -50.0
        else:
            xi[ch, t0, 2] = np.nan
    return xi, g, gl


def tstat_deviation(got, ref, n):
    """NC.tstat_deviation over the rows whose reference is finite; the others must be equal (-inf)
    or NaN on both sides."""
    got, ref = np.asarray(got), np.asarray(ref)
    fin = np.isfinite(ref.astype(np.float64))
    odd_ok = np.array_equal(got[~fin].astype(np.float64), ref[~fin].astype(np.float64), equal_nan=True)
    return NC.tstat_deviation(got[fin], ref[fin], n) if odd_ok else np.inf


# ---- device RNG -------------------------------------------------------------------------------------
def _streams(seed, n, k, nu, nu0, sweeps):
    """xi, g, gl of a device-RNG chain restated on the host, and the smallest accept / reject margin
    of the two gamma streams."""
    xi = R.normals(seed, sweeps * k).astype(np.float64).reshape(sweeps, k)
    g, _, mg = R.gammas(seed, (nu0 + n) / 2, sweeps)
    gl, attempts, ml = RR.robust_gammas(seed, nu, n, sweeps)
    assert attempts.max() < 64
    return xi, g, gl, float(min(mg.min(), ml.min()))


@functools.lru_cache(maxsize=None)
def burn_device_reference(dtype=LD):
    """Section B: RC.device_problem(), nu = 4, burn 37, 50 kept sweeps, fed the host-restated streams:
    a list of (samples, weights, margin) per seed."""
    y, X, prior = RC.device_problem()
    out = []
    for seed in BURN_DEVICE_SEEDS:
        xi, g, gl, margin = _streams(seed, RC.DEVICE_N, RC.DEVICE_K, RC.DEVICE_NU, prior[2],
                                     BURN_DEVICE_BURN + BURN_DEVICE_ITERS)
        s, w = RR.chain(y, X, BURN_DEVICE_ITERS, prior, RC.DEVICE_NU, xi, g, gl, burn=BURN_DEVICE_BURN, dtype=dtype)
        out.append((s, w, margin))
    return out


@functools.lru_cache(maxsize=None)
def low_reference(dtype=LD):
    """Section F, fixed nu = 0.5 (shape 0.75, the boosted branch): a list of (samples, weights, margin)."""
    y, X, prior = low_problem()
    out = []
    for seed in LOW_SEEDS:
        xi, g, gl, margin = _streams(seed, LOW_N, LOW_K, LOW_NU, prior[2], LOW_T)
        s, w = RR.chain(y, X, LOW_T, prior, LOW_NU, xi, g, gl, dtype=dtype)
        out.append((s, w, margin))
    return out


@functools.lru_cache(maxsize=None)
def low_nu_reference(dtype=LD):
    """Section F on the grid LOW_GRID: free chains fed the host-restated streams, the construction of
    robust_nu_cases.device_reference: a list of (NR.chain dict, the smallest Marsaglia-Tsang margin
    along the chain's own path)."""
    y, X, prior = low_problem()
    out = []
    for seed in LOW_NU_SEEDS:
        xi, g, tabs, margins, u = NR.device_streams(seed, LOW_N, LOW_K, LOW_T, LOW_GRID, prior[2])
        r = NR.chain(y, X, LOW_T, prior, LOW_GRID, LOW_WEIGHT, LOW_INIT, xi, g, lambda t, gi: tabs[gi, t], u,
                     dtype=dtype)
        before = np.concatenate([[LOW_INIT], r["path"][:-1]])
        out.append((r, float(margins[before, np.arange(LOW_T)].min())))
    return out


# ---- the deviations REF_DEV records -----------------------------------------------------------------
def _pair_dev(f64, ld):
    """max over chains of (samples, weights) deviations of (samples (C, ..), weights (C, ..)) pairs."""
    return (max(RC.scaled_deviation(a, b) for a, b in zip(f64[0], ld[0])),
            max(RC.weight_deviation(a, b) for a, b in zip(f64[1], ld[1])))


def _nu_dev(f64, ld, n):
    return (max(RC.scaled_deviation(a["samples"], b["samples"]) for a, b in zip(f64, ld)),
            max(RC.weight_deviation(a["weights"], b["weights"]) for a, b in zip(f64, ld)),
            max(tstat_deviation(a["tstat"], b["tstat"], n) for a, b in zip(f64, ld)))


def ref_dev_names():
    return [f"{n}x{k}" for n, k in SHAPES] + ["C"] + list(NU_CASES) + ["F-fixed", "F-nu"]


def recompute_ref_dev(name):
    """The float64 reference against the long-double one on the case ``name`` of REF_DEV."""
    if name == "C":
        return _pair_dev(floor_reference(np.float64), floor_reference())
    if name in NU_CASES:
        return _nu_dev(nu_reference(name, np.float64), nu_reference(name), nu_case(name)["n"])
    if name == "F-fixed":
        f64, ld = low_reference(np.float64), low_reference()
        return _pair_dev(([r[0] for r in f64], [r[1] for r in f64]), ([r[0] for r in ld], [r[1] for r in ld]))
    if name == "F-nu":
        return _nu_dev([r for r, _ in low_nu_reference(np.float64)], [r for r, _ in low_nu_reference()], LOW_N)
    n, k = (int(v) for v in name.split("x"))
    return _pair_dev(fixed_reference(n, k, np.float64), fixed_reference(n, k))
