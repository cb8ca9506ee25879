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
    p_value[j]     mean_s 1[T_rep[s, j] >= T_obs[s, j]]  (a NaN is never >=)

A value is NaN exactly where these definitions give NaN (numpy's min and max propagate a NaN), and
all ten per-draw values of a draw with a non-finite coefficient or without a finite sigma > 0 are
NaN.  ``reference(..., dtype=np.float64)`` is the same text in float64 (two-pass moments), for the
rounding floors FLOORS at the end of the file.
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


def marginal(x, dtype=LD):
    """(6, ...) ``dtype``: min, max, mean, sd, skew, kurt over axis 0 (two passes: the mean, then the
    moments of the deviations).  A NaN among the values makes all six NaN."""
    x = np.asarray(x, dtype=dtype)
    with np.errstate(all="ignore"):
        mean = x.mean(axis=0)
        d = x - mean
        m2, m3, m4 = ((d ** r).mean(axis=0) for r in (2, 3, 4))
        return np.stack([x.min(axis=0), x.max(axis=0), mean, np.sqrt(m2), m3 / m2 ** dtype(1.5),
                         m4 / m2 ** 2 - dtype(3)])


def bad_draws(theta):
    """(S,) bool: the draws with a non-finite coefficient or without a finite sigma > 0.  All ten
    values of such a draw are NaN (as psis_reference and sens_reference treat it)."""
    th = np.asarray(theta, dtype=np.float64)
    return ~(np.isfinite(th).all(axis=1) & (th[:, -1] > 0))


def reference(A, y, theta, seed, offset=None, dtype=LD, z_factor=None):
    """(t_rep, t_obs), both (S, 8) ``dtype``: long double, or float64 for the rounding floor (the
    long-double variates rounded once, everything after them in float64).  ``z_factor`` (n, S)
    multiplies the variates: the floor test's stand-in for the device generator's accuracy."""
    A = np.asarray(A, dtype=dtype)
    y = np.asarray(y, dtype=dtype)
    th = np.asarray(theta, dtype=dtype)
    n, k = A.shape
    S = th.shape[0]
    off = np.zeros(n, dtype=dtype) if offset is None else np.asarray(offset, dtype=dtype)
    z = noise(seed, n, np.arange(S))
    if z_factor is not None:
        z = z * np.asarray(z_factor, dtype=LD)
    z = z.astype(dtype)
    t_rep = np.empty((S, 8), dtype=dtype)
    t_obs = np.empty((S, 8), dtype=dtype)
    with np.errstate(all="ignore"):
        if dtype is LD:
            mu = A @ th[:, :k].T                   # (n, S)
        else:                                      # numpy's own pairwise sum, not a BLAS order
            mu = (A[:, None, :] * th[None, :, :k]).sum(axis=2)
        sg = th[:, k][None, :]
        yrep = mu + sg * z + off[:, None]
        e = (y[:, None] - mu) / sg
        t_rep[:, :6] = marginal(yrep, dtype).T
        t_rep[:, 6] = (z * z).sum(axis=0)
        t_rep[:, 7] = np.abs(z).max(axis=0)
        t_obs[:, :6] = marginal(y + off, dtype)[None, :]
        t_obs[:, 6] = (e * e).sum(axis=0)
        t_obs[:, 7] = np.abs(e).max(axis=0)
    bad = bad_draws(theta)
    t_rep[bad] = np.nan
    t_obs[bad, 6:] = np.nan
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


# ---- the shape grid (tests/test_ppc_gpu.py::test_shapes_on_both_sides_of_every_rule) ----------------
# Points on both sides of the 64-point tile and of the Box-Muller partner at i + 32 (31, 32, 33: the
# partner of the last point does not exist), the full-tile branch exactly (64, 128); k at and around
# the 16-column slab (16 and 32: k_pad == k, no spare slab column) up to the limit; draws around
# the 64-draw tile.  Every noise seed has a non-zero high word.
GRID_N = (31, 32, 33, 63, 64, 65, 127, 128, 129)
GRID_K = (1, 15, 16, 17, 32, 33, 64, 256)
GRID_S = (2, 63, 64, 65, 129)


def grid_noise_seed(data_seed):
    return (0x9E3779B9 << 32) | (data_seed * 2654435761 % 2 ** 32)


def grid_shapes(k):
    """(case, n, S, seed of the data), case counting n-major."""
    return [(ni * len(GRID_S) + si, n, S, 40000 + 100 * k + ni * len(GRID_S) + si)
            for ni, n in enumerate(GRID_N) for si, S in enumerate(GRID_S)]


def grid_offset(case, n, data_seed):
    """Every third case has an offset."""
    if case % 3:
        return None
    return 1.0 + 0.5 * np.random.default_rng(data_seed + 7).standard_normal(n)


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def grid_case(k, case):
    """(n, S, A, y, theta, offset or None, noise seed, t_rep, t_obs); computed once, never changed."""
    key = ("grid", k, case)
    if key not in _CACHE:
        c, n, S, data_seed = grid_shapes(k)[case]
        A, y, th = make_case(n, k, S, data_seed)
        off = grid_offset(case, n, data_seed)
        seed = grid_noise_seed(data_seed)
        t_rep, t_obs = reference(A, y, th, seed, offset=off)
        _CACHE[key] = (n, S) + _frozen(A, y, th, off) + (seed,) + _frozen(t_rep, t_obs)
    return _CACHE[key]


# The first and the last key: the data of CASES[3] under noise seeds 0 and 2^64 - 1
SEED_EDGES = (0, 2 ** 64 - 1)


def seed_edge_case(seed):
    """As grid_case: (n, S, A, y, theta, None, seed, t_rep, t_obs)."""
    key = ("seed", seed)
    if key not in _CACHE:
        A, y, th = case(65, 3, 130, 11)[:3]
        t_rep, t_obs = reference(A, y, th, seed)
        _CACHE[key] = (65, 130, A, y, th, None, seed) + _frozen(t_rep, t_obs)
    return _CACHE[key]


def offset_case():
    """CASES[4] with an offset of 20 + 5 N, as grid_case (test_offset_moves_the_marginal_statistics_only)."""
    key = ("offset",)
    if key not in _CACHE:
        A, y, th, seed = case(150, 17, 64, 13)[:4]
        off = 20.0 + 5.0 * np.random.default_rng(1).standard_normal(150)
        t_rep, t_obs = reference(A, y, th, seed, offset=off)
        _CACHE[key] = (150, 64, A, y, th) + _frozen(off) + (seed,) + _frozen(t_rep, t_obs)
    return _CACHE[key]


# ---- biased fits -------------------------------------------------------------------------------------
# An intercept column, data at level 5 with sd(y_rep) about 0.02, and draws whose intercept is off by
# delta: the replicated mean sits delta / 0.02 = 15 or 150 sd from mean(y).  One-pass moments about
# any centre that all draws share lose (delta / sd)^4 u of kurt here; a predictive check exists to
# flag exactly such a fit.
BIASED = (0.3, 3.0)
BIASED_SD = {0.3: 10.0, 3.0: 150.0}        # the replicated mean is further than this from mean(y)
BIASED_SEED = (7 << 32) | 5


def make_biased(delta):
    rng = np.random.default_rng(91)
    n, S = 200, 64
    A = np.column_stack([np.ones(n), rng.standard_normal(n)])
    y = 5 + 0.02 * A[:, 1] + 0.01 * rng.standard_normal(n)
    th = np.empty((S, 3))
    th[:, 0] = 5 + delta + 0.001 * rng.standard_normal(S)
    th[:, 1] = 0.02 + 0.001 * rng.standard_normal(S)
    th[:, 2] = 0.01 * np.exp(0.05 * rng.standard_normal(S))
    return A, y, th


def biased_case(delta):
    """As grid_case: (n, S, A, y, theta, None, seed, t_rep, t_obs)."""
    key = ("biased", delta)
    if key not in _CACHE:
        A, y, th = make_biased(delta)
        t_rep, t_obs = reference(A, y, th, BIASED_SEED)
        _CACHE[key] = (200, 64) + _frozen(A, y, th, None) + (BIASED_SEED,) + _frozen(t_rep, t_obs)
    return _CACHE[key]


# ---- floors and bars ---------------------------------------------------------------------------------
# Ten values per draw: the eight of t_rep and the two observed ones that depend on the draw.
TEN = PPC_STATS + ("chi2_obs", "max_abs_e")
GROUPS = ("cases", "grid", "biased")
Z_ACCURACY = 2.1 * 2.0 ** -52            # the device's variates against rng_reference


def group_cases(group):
    """The (n, S, A, y, theta, offset, seed, t_rep, t_obs) of every case of a group."""
    if group == "cases":
        for c in CASES:
            A, y, th, seed, t_rep, t_obs = case(*c)
            yield (c[0], c[2], A, y, th, None, seed, t_rep, t_obs)
        yield offset_case()
    elif group == "grid":
        for k in GRID_K:
            for c in range(len(GRID_N) * len(GRID_S)):
                yield grid_case(k, c)
        for seed in SEED_EDGES:
            yield seed_edge_case(seed)
    else:
        for delta in BIASED:
            yield biased_case(delta)


def ten(t_rep, t_obs):
    """(S, 10): t_rep and the two per-draw columns of t_obs side by side, the order of TEN."""
    return np.concatenate([np.asarray(t_rep), np.asarray(t_obs)[:, 6:]], axis=1)


def deviation(got, ref):
    """(10,) float64: the largest |got - ref| / max(1, |ref|) per value of TEN; ref long double."""
    ref = np.asarray(ref, dtype=LD)
    e = np.abs(np.asarray(got, dtype=LD) - ref) / np.maximum(LD(1), np.abs(ref))
    return e.max(axis=0).astype(np.float64)


def measured_floors(group):
    """(10,) float64: per value of TEN over the group's cases, the larger of (a) the float64
    reference's deviation from the long-double one and (b) the long-double reference with every z
    replaced by z (1 + d), |d| = Z_ACCURACY with random signs, against the unperturbed one.  Neither
    involves the device."""
    worst = np.zeros(len(TEN))
    rng = np.random.default_rng(2024)
    for n, S, A, y, th, off, seed, t_rep, t_obs in group_cases(group):
        ref = ten(t_rep, t_obs)
        f64 = ten(*reference(A, y, th, seed, offset=off, dtype=np.float64))
        fac = 1 + Z_ACCURACY * rng.choice([-1.0, 1.0], size=(n, S)).astype(LD)
        pert = ten(*reference(A, y, th, seed, offset=off, z_factor=fac))
        worst = np.maximum(worst, np.maximum(deviation(f64, ref), deviation(pert, ref)))
    return worst


# measured_floors() of each group, rounded up to two digits; tests/test_ppc_host.py recomputes them
# and asserts that none exceeds its constant.  Measured in units of 1e-16 (the order of TEN):
#   cases    3.63  3.24  12.8  10.2   121    146   18.6  4.66  23.3  22.9   (CASES and offset_case)
#   grid     14.0  15.7  32.7  6.71   35.5   86.6  11.7  4.66  354   413
#   biased   1.37  2.04  11.3  1.33   9970   3180  13.5  4.66  9.99  13.9
# (biased skew and kurt: |y_rep| / sd is about 250, which forming y_rep in float64 pays for whatever
# comes after.)
FLOORS = {
    "cases": (3.7e-16, 3.3e-16, 1.3e-15, 1.1e-15, 1.3e-14, 1.5e-14, 1.9e-15, 4.7e-16, 2.4e-15, 2.3e-15),
    "grid": (1.5e-15, 1.6e-15, 3.3e-15, 6.8e-16, 3.6e-15, 8.7e-15, 1.2e-15, 4.7e-16, 3.6e-14, 4.2e-14),
    "biased": (1.4e-16, 2.1e-16, 1.2e-15, 1.4e-16, 1.0e-12, 3.2e-13, 1.4e-15, 4.7e-16, 1.0e-15, 1.4e-15),
}
BAR_FACTOR = 64          # the MFMA's and the lane tree's summation order, the one-pass
#                          moments, and exp / log / sincos that are not correctly rounded


def round_up_one_digit(x):
    """The smallest d * 10^e >= x with d in 1 .. 9 (decimal arithmetic: 64 * 1.5e-15 is 9.6e-14)."""
    from decimal import ROUND_CEILING, Decimal
    d = Decimal(repr(float(x)))
    return float(d.quantize(Decimal(1).scaleb(d.adjusted()), rounding=ROUND_CEILING))


def bars(group):
    """{name of TEN: bar}: BAR_FACTOR x the floor, rounded up to one significant digit."""
    return {name: round_up_one_digit(BAR_FACTOR * f) for name, f in zip(TEN, FLOORS[group])}
