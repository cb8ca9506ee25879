"""Problems, grids, paths and variates shared by the tests of the Student-t sampler with nu on a grid
(test_robust_nu_host.py on the CPU, test_robust_nu_gpu.py on the GPU).  TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

import robust_cases as RC
import robust_nu_reference as NR

# replay parity: the smallest shapes per kernel width and slab edge
#   3 x 2 KC = 4;  65 x 1 a slab one past a wave;  257 x 17 KC = 32, a ragged last k-step;
#   64 x 16 KC = 16;  300 x 8 KC = 8
REPLAY_CASES = ((3, 2), (65, 1), (257, 17), (64, 16), (300, 8))
T = 300
CHAINS = 3
GRID = np.array([1.5, 2.5, 4.0, 7.0, 12.0, 25.0, 50.0])
WEIGHT = np.array([1.0, 2.0, 3.0, 3.0, 2.0, 1.0, 0.5])
NU_INIT = 2
# device RNG: (N, k) -> the chains' seeds (test_robust_nu_host.py proves their margins)
DEVICE_CASES = {(65, 1): (30101, 30102, 30103), (300, 8): (30201, 30202, 30203)}


def problem(n, k):
    """(y, X, prior) of tests/robust_cases.py: its goldens and its synthetic recipe."""
    return RC.problem(n, k)


@functools.lru_cache(maxsize=None)
def replay_inputs(n, k):
    """paths (C, T) int32 and the variates xi (C, T, k), g (C, T), gl (C, T, N), u (C, T)."""
    nu0 = problem(n, k)[2][2]
    paths = np.stack([NR.forced_path(len(GRID), T, c) for c in range(CHAINS)])
    parts = [NR.path_variates(n, k, T, GRID, NU_INIT, paths[c], nu0, seed=104729 * n + 37 * k + c)
             for c in range(CHAINS)]
    return (paths,) + tuple(np.stack([p[i] for p in parts]) for i in range(4))


@functools.lru_cache(maxsize=None)
def replay_reference(n, k, dtype=np.longdouble):
    """The reference's chains on the forced paths: a list of NR.chain dicts."""
    y, X, prior = problem(n, k)
    paths, xi, g, gl, u = replay_inputs(n, k)
    return [NR.chain(y, X, T, prior, GRID, WEIGHT, NU_INIT, xi[c], g[c], gl[c], u[c], dtype=dtype,
                     path=paths[c]) for c in range(CHAINS)]


@functools.lru_cache(maxsize=None)
def device_reference(n, k, dtype=np.longdouble):
    """Free chains fed the host-restated streams of DEVICE_CASES[(n, k)]: a list of (NR.chain dict,
    the smallest Marsaglia-Tsang accept margin along the chain's own path)."""
    y, X, prior = problem(n, k)
    out = []
    for seed in DEVICE_CASES[(n, k)]:
        xi, g, tabs, margins, u = NR.device_streams(seed, n, k, T, GRID, prior[2])
        r = NR.chain(y, X, T, prior, GRID, WEIGHT, NU_INIT, xi, g, lambda t, gi: tabs[gi, t], u, dtype=dtype)
        before = np.concatenate([[NU_INIT], r["path"][:-1]])
        out.append((r, float(margins[before, np.arange(T)].min())))
    return out


def tstat_deviation(got, ref, n):
    """T_t is a sum over n rows: max |got - ref| / n."""
    return float(np.max(np.abs(np.asarray(got, dtype=np.longdouble) - ref)) / n)


def t_noise_problem(n, k, df, seed):
    """y = X beta + 0.3 e with e ~ t_df (df = None: normal), X standard normal."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, k))
    e = rng.standard_normal(n) if df is None else rng.standard_t(df, n)
    y = X @ np.arange(1.0, k + 1.0) + 0.3 * e
    return y, X, (np.zeros(k), 25.0 * np.eye(k), 1.0, 0.02)


def free_reference(y, X, prior, grid, weight, init, burn, keep, seed):
    """A float64 reference chain on numpy variates drawn sweep by sweep at the shape in force."""
    n, k = X.shape
    rng = np.random.default_rng(seed)
    sweeps = burn + keep
    xi = rng.standard_normal((sweeps, k))
    g = rng.gamma((prior[2] + n) / 2, size=sweeps)
    u = rng.random(sweeps)
    return NR.chain(y, X, keep, prior, grid, weight, init, xi, g,
                    lambda t, gi: rng.gamma((grid[gi] + 1.0) / 2.0, size=n), u, burn=burn)
