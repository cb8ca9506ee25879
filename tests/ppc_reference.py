"""The posterior predictive check restated on the host.  TEST INFRASTRUCTURE ONLY.

numpy.longdouble and nothing of the kernel's text: the definitions of pybmc_amd/ppc.py's
docstring, the fifth variate stream built on rng_reference (Philox4x32-10, the uniforms and the
Box-Muller transform of the other four streams):

    z[i, s]        the Box-Muller pair of counter (s lo, s hi, STREAM_PPC, pair(i)) under key = seed,
                   pair(i) = (i >> 6) * 32 + (i & 31); the cosine half when (i >> 5) & 1 == 0, else
                   the sine half (so points i and i + 32 of a 64-point tile share a counter)
    y_rep[i, s]    a_i . beta_s + sigma_s z[i, s] + offset_i
    T_rep[s, :]    min, max, mean, sd, skew, kurt of y_rep[:, s] (moments about the mean, ddof 0),
                   sum_i z^2, max_i |z|
    T_obs[s, :]    the same six of y + offset, then sum_i e^2 and max_i |e|,
                   e = (y_i - a_i . beta_s) / sigma_s
    p_value[j]     mean_s 1[T_rep[s, j] >= T_obs[s, j]]
"""
import numpy as np

import rng_reference as G

LD = np.longdouble
STREAM_PPC = 0x50504353          # "PPCS"
PPC_STATS = ("min", "max", "mean", "sd", "skew", "kurt", "chi2", "max_abs_z")
MARGIN_FLOOR = G.MARGIN_FLOOR

# The cases of tests/test_ppc_gpu.py: (n, k, S, seed of the data).  tests/test_ppc_host.py proves on
# the CPU that no T_rep of theirs sits within MARGIN_FLOOR of its T_obs, which is what lets the GPU
# test demand equal p-values.  (4, 1, 2) stands beside (3, 1, 2) because the kurtosis of ANY three
# values is -3/2: with d = (a, b, -a - b), sum d^4 = 2 (a^2 + a b + b^2)^2 and sum d^2 =
# 2 (a^2 + a b + b^2), so m4 / m2^2 = 3/2.  At n = 3 T_rep and T_obs of kurt are the same number and
# their comparison is a tie that rounding decides: DEGENERATE names that pair, which is checked as
# a value (both -3/2) and left out of the margin and p-value comparisons; n = 4 is the smallest
# size at which all eight are compared.
CASES = ((3, 1, 2, 5), (4, 1, 2, 23), (33, 1, 70, 7), (65, 3, 130, 11), (150, 17, 64, 13),
         (200, 33, 257, 17), (629, 3, 300, 19))
DEGENERATE = {3: ("kurt",)}


def noise_seed(seed):
    return 1000 + seed


def make_case(n, k, S, seed, noise=0.3):
    """Gaussian design, y = A beta + noise * eps; draws = the least-squares coefficients + 0.05 N,
    sigma = 0.3 exp(0.05 N) (so ``noise = 0.3`` is a well-specified fit).  Returns A, y, theta."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, k))
    y = A @ rng.standard_normal(k) + noise * rng.standard_normal(n)
    bh = np.linalg.lstsq(A, y, rcond=None)[0]
    th = np.empty((S, k + 1))
    th[:, :k] = bh + 0.05 * rng.standard_normal((S, k))
    th[:, k] = 0.3 * np.exp(0.05 * rng.standard_normal(S))
    return A, y, th


def pair_index(i):
    i = np.asarray(i, dtype=np.uint64)
    return (i >> np.uint64(6)) * np.uint64(32) + (i & np.uint64(31))


def half_index(i):
    return ((np.asarray(i, dtype=np.uint64) >> np.uint64(5)) & np.uint64(1)).astype(np.int64)


def noise_counters(n, draws):
    """(index (n, S), sub (n, 1)) of the counters (index lo, index hi, STREAM_PPC, sub)."""
    draws = np.asarray(draws, dtype=np.uint64)
    index = np.broadcast_to(draws[None, :], (n, len(draws)))
    return index, pair_index(np.arange(n))[:, None]


def noise(seed, n, draws):
    """(n, len(draws)) long double: z[i, s] for the draw indices ``draws``."""
    index, sub = noise_counters(n, draws)
    u1, u2 = G.pair_uniforms(G.stream_words(seed, index, STREAM_PPC, sub))
    z0, z1, _ = G.box_muller(u1, u2)
    return np.where(half_index(np.arange(n))[:, None] == 1, z1, z0)


def marginal(x):
    """(6, ...) long double: min, max, mean, sd, skew, kurt over axis 0."""
    x = np.asarray(x, dtype=LD)
    mean = x.mean(axis=0)
    d = x - mean
    m2, m3, m4 = ((d ** r).mean(axis=0) for r in (2, 3, 4))
    return np.stack([x.min(axis=0), x.max(axis=0), mean, np.sqrt(m2), m3 / m2 ** LD(1.5),
                     m4 / m2 ** 2 - LD(3)])


def reference(A, y, theta, seed, offset=None):
    """(t_rep, t_obs), both (S, 8) long double."""
    A = np.asarray(A, dtype=LD)
    y = np.asarray(y, dtype=LD)
    th = np.asarray(theta, dtype=LD)
    n, k = A.shape
    S = th.shape[0]
    off = np.zeros(n, dtype=LD) if offset is None else np.asarray(offset, dtype=LD)
    mu = A @ th[:, :k].T                       # (n, S)
    sg = th[:, k][None, :]
    z = noise(seed, n, np.arange(S))
    yrep = mu + sg * z + off[:, None]
    e = (y[:, None] - mu) / sg
    t_rep = np.empty((S, 8), dtype=LD)
    t_obs = np.empty((S, 8), dtype=LD)
    t_rep[:, :6] = marginal(yrep).T
    t_rep[:, 6] = (z * z).sum(axis=0)
    t_rep[:, 7] = np.abs(z).max(axis=0)
    t_obs[:, :6] = marginal(y + off)[None, :]
    t_obs[:, 6] = (e * e).sum(axis=0)
    t_obs[:, 7] = np.abs(e).max(axis=0)
    return t_rep, t_obs


def p_values(t_rep, t_obs):
    return {name: float(np.mean(t_rep[:, j] >= t_obs[:, j])) for j, name in enumerate(PPC_STATS)}


def margins(t_rep, t_obs):
    """(S, 8) float64: |T_rep - T_obs| / max(1, |T_rep|, |T_obs|)."""
    scale = np.maximum(LD(1), np.maximum(np.abs(t_rep), np.abs(t_obs)))
    return (np.abs(t_rep - t_obs) / scale).astype(np.float64)


def compared(n):
    """Indices of the statistics whose T_rep and T_obs are compared at this n (see DEGENERATE)."""
    return [j for j, name in enumerate(PPC_STATS) if name not in DEGENERATE.get(n, ())]


_CACHE = {}


def case(n, k, S, seed):
    """(A, y, theta, noise seed, t_rep, t_obs) of a case of CASES; computed once, never changed."""
    key = (n, k, S, seed)
    if key not in _CACHE:
        A, y, th = make_case(n, k, S, seed)
        t_rep, t_obs = reference(A, y, th, noise_seed(seed))
        for a in (A, y, th, t_rep, t_obs):
            a.setflags(write=False)
        _CACHE[key] = (A, y, th, noise_seed(seed), t_rep, t_obs)
    return _CACHE[key]
