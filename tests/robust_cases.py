"""Problems and variates shared by the Student-t sampler's tests (test_robust_host.py on the CPU,
test_robust_gpu.py on the GPU).  TEST INFRASTRUCTURE ONLY."""
import functools
import os

import numpy as np

import robust_reference as RR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# replay parity: (N, k) -> golden fixture or None (a dense synthetic problem); three of them are not
# orthonormal by construction (the synthetic ones and the tiny / ragged goldens)
REPLAY_CASES = {(3, 2): "gibbs_tiny3x2", (65, 1): None, (64, 16): None, (257, 17): None,
                (629, 3): "gibbs_ortho629x3", (1237, 5): "gibbs_ragged1237x5", (300, 32): None}
REPLAY_NUS = (1.5, 4.0, 50.0)
REPLAY_T = 300
REPLAY_CHAINS = 3

# the planted-outlier problems of the host and device statistics tests: (N, k, share, seed)
PLANTED = {"200x3": (200, 3, 0.05, 11), "333x8": (333, 8, 0.06, 12)}
PLANTED_BURN, PLANTED_KEEP = 200, 1800
# seeds of the device-RNG runs; test_robust_host.py proves no STREAM_ROBUST attempt of DEVICE_SEEDS
# on the 65 x 3 case lies within 1e-9 of an accept / reject boundary
DEVICE_SEEDS = (20261, 20262)
DEVICE_N, DEVICE_K, DEVICE_T, DEVICE_NU = 65, 3, 50, 4.0


def _golden(name):
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        return (np.array(z["y"], dtype=np.float64), np.array(z["X"], dtype=np.float64),
                (np.array(z["b0"]), np.array(z["C0"]), float(z["nu0"]), float(z["s20"])))


@functools.lru_cache(maxsize=None)
def problem(n, k):
    """(y, X, prior) of a replay case.  The synthetic ones: a dense X with correlated columns, a
    tenth of the rows moved by several sigma."""
    name = REPLAY_CASES.get((n, k))
    if name is not None:
        return _golden(name)
    rng = np.random.default_rng(1000 * n + k)
    X = rng.standard_normal((n, k)) + 0.3 * rng.standard_normal((n, 1))
    beta = rng.standard_normal(k)
    y = X @ beta + 0.5 * rng.standard_normal(n)
    bad = rng.choice(n, max(1, n // 10), replace=False)
    y[bad] += 5.0 * rng.standard_normal(len(bad))
    return y, X, (np.zeros(k), 4.0 * np.eye(k), 1.0, 0.02)


@functools.lru_cache(maxsize=None)
def replay_variates(n, k, nu):
    """xi (C, T, k), g (C, T), gl (C, T, N): three chains with different variates."""
    nu0 = problem(n, k)[2][2]
    parts = [RR.host_variates(n, k, REPLAY_T, nu, nu0, seed=7919 * n + 31 * k + 3 * c + int(10 * nu))
             for c in range(REPLAY_CHAINS)]
    return tuple(np.stack([p[i] for p in parts]) for i in range(3))


@functools.lru_cache(maxsize=None)
def replay_reference(n, k, nu, dtype=np.longdouble):
    """(samples (C, T, k + 1), weights (C, N)) of the reference in ``dtype``."""
    y, X, prior = problem(n, k)
    xi, g, gl = replay_variates(n, k, nu)
    runs = [RR.chain(y, X, REPLAY_T, prior, nu, xi[c], g[c], gl[c], dtype=dtype)
            for c in range(REPLAY_CHAINS)]
    return np.stack([r[0] for r in runs]), np.stack([r[1] for r in runs])


def scaled_deviation(got, ref):
    """max |got - ref| relative to each column's scale max |ref| (columns: the last axis)."""
    ref = np.asarray(ref)
    flat = ref.reshape(-1, ref.shape[-1])
    scale = np.abs(flat).max(axis=0).astype(np.float64)
    diff = np.abs(np.asarray(got, dtype=np.longdouble) - ref).reshape(flat.shape).max(axis=0)
    return float(np.max(diff.astype(np.float64) / scale))


def weight_deviation(got, ref):
    """The row weights of a chain are one column: max |got - ref| / max |ref|."""
    ref = np.asarray(ref)
    return float(np.max(np.abs(np.asarray(got, dtype=np.longdouble) - ref)) / np.max(np.abs(ref)))


@functools.lru_cache(maxsize=None)
def planted(name):
    n, k, frac, seed = PLANTED[name]
    return RR.planted_problem(n, k, frac, seed)


def device_problem():
    """The 65 x 3 problem of the device-RNG test."""
    rng = np.random.default_rng(65003)
    X = rng.standard_normal((DEVICE_N, DEVICE_K))
    y = X @ np.array([1.0, -2.0, 0.5]) + 0.3 * rng.standard_normal(DEVICE_N)
    y[[5, 40]] += 4.0
    return y, X, (np.zeros(DEVICE_K), 4.0 * np.eye(DEVICE_K), 1.0, 0.02)
