"""The posterior predictive check with Student-t replicated noise restated on the host.  TEST
INFRASTRUCTURE ONLY.

numpy.longdouble and nothing of the kernel's text.  The variates are Bailey's polar form on the
eighth variate stream, built on rng_reference's Philox4x32-10 and uniforms:

    z[i, s]   sqrt(nu_s expm1(-(2 / nu_s) log u1)) cos(2 pi u2), (u1, u2) the two uniforms of counter
              (s lo, s hi, STREAM_PPC_T, i) under key = seed: the point index itself, and the cosine
              half alone (the sine half shares the radius: test_ppc_t_host.py shows what that does)

and everything after z is ppc_reference.reference, unchanged: y_rep = a_i . beta_s + sigma_s z +
offset_i, the eight T_rep, the T_obs with e = (y_i - a_i . beta_s) / sigma_s, the NaN rules.

T_ACCURACY plays the part of ppc_reference.Z_ACCURACY: the largest relative deviation of
student_t_variate (bmc_math.h, the text the kernels compile, built by g++) from a long-double
restatement, per nu, over u1 from 2^-53 to 1 (tests/ppc_t_math_check.cpp, line 3 of its output;
tests/test_ppc_t_host.py asserts that the measurement stays below these).  It grows as nu falls:
the radius is exp(x / 2) with x = -(2 / nu) log u1 up to 73.5 / nu, and a relative error d of x --
the logarithm's, or that of 2 / nu rounded to a double -- is an error x d / 2 of the radius.
Measured: 4.73e-15, 1.16e-15, 4.85e-16 for nu = 1.5, 4, 50.
"""
import contextlib

import numpy as np

import ppc_reference as P
import rng_reference as G

LD = np.longdouble
STREAM_PPC_T = 0x50504354          # "PPCT"
NUS = (1.5, 4.0, 50.0)
T_ACCURACY = {1.5: 22.0 * 2.0 ** -52, 4.0: 5.4 * 2.0 ** -52, 50.0: 2.3 * 2.0 ** -52}
MARGIN_FLOOR = P.MARGIN_FLOOR
TEN = P.TEN
BAR_FACTOR = P.BAR_FACTOR
_PI_2 = LD("1.5707963267948966192313216916397514421")


def cos_2pi(u2):
    """cos(2 pi u2) in long double: 4 u2 = q + r with q the nearest integer is exact in float64,
    the cosine or sine of (pi/2) r moved to the quadrant (as rng_reference.box_muller)."""
    t = 4.0 * np.asarray(u2, dtype=np.float64)
    q = np.rint(t)
    x = (t - q).astype(LD) * _PI_2
    iq = q.astype(np.int64) & 3
    b = np.where((iq & 1) == 1, np.sin(x), np.cos(x))
    return np.where(((iq + 1) & 2) != 0, -b, b)


def radius(u1, nu):
    nu = np.asarray(nu, dtype=LD)
    return np.sqrt(nu * np.expm1(-(LD(2) / nu) * np.log(np.asarray(u1).astype(LD))))


def t_variate(u1, u2, nu):
    """(cosine half, sine half) of Bailey's polar pair, long double.  The product uses the first."""
    rad = radius(u1, nu)
    t = 4.0 * np.asarray(u2, dtype=np.float64)
    q = np.rint(t)
    x = (t - q).astype(LD) * _PI_2
    iq = q.astype(np.int64) & 3
    a = np.where((iq & 1) == 1, np.cos(x), np.sin(x))
    sn = np.where((iq & 2) != 0, -a, a)
    return rad * cos_2pi(u2), rad * sn


def nu_of_draws(nu, S):
    """(S,) float64: one nu for all draws, or the given one per draw."""
    nu = np.asarray(nu, dtype=np.float64)
    return np.full(S, float(nu)) if nu.ndim == 0 else nu.reshape(S)


def uniforms(seed, n, draws):
    """(u1, u2), both (n, len(draws)) float64, of points 0 .. n-1 and the draw indices ``draws``."""
    draws = np.asarray(draws, dtype=np.uint64)
    index = np.broadcast_to(draws[None, :], (n, len(draws)))
    sub = np.arange(n, dtype=np.uint64)[:, None]
    return G.pair_uniforms(G.stream_words(seed, index, STREAM_PPC_T, sub))


def noise(seed, n, draws, nu):
    """(n, len(draws)) long double: z[i, s] for the draw indices ``draws``; ``nu`` one value or one
    per entry of ``draws``."""
    u1, u2 = uniforms(seed, n, draws)
    return t_variate(u1, u2, nu_of_draws(nu, len(draws))[None, :])[0]


@contextlib.contextmanager
def _noise_of(nu):
    """ppc_reference.reference with this file's variates in the place of its normals."""
    saved = P.noise
    P.noise = lambda seed, n, draws: noise(seed, n, draws, nu)
    try:
        yield
    finally:
        P.noise = saved


def reference(A, y, theta, seed, nu, offset=None, dtype=LD, z_factor=None):
    """(t_rep, t_obs) as ppc_reference.reference, the noise Student-t with ``nu`` (one value, or one
    per draw) degrees of freedom."""
    with _noise_of(nu):
        return P.reference(A, y, theta, seed, offset=offset, dtype=dtype, z_factor=z_factor)


# ---- the cases of tests/test_ppc_t_gpu.py ------------------------------------------------------------
# (n, k, S, nu or "cycle", noise seed, offset?): every n of {3, 63, 64, 65, 129} (the 64-point tile
# edge, on which nothing at i + 32 may depend), every k of {1, 16, 17}, every S of {2, 64, 65, 130},
# every nu of NUS, nu per draw cycling through NUS (so a 64-draw tile holds all three and the cycle
# crosses the tile edge at S = 65 and 130), the first and the last key, keys with a non-zero high word.
HI = 0x9E3779B9 << 32
CYCLE = "cycle"
CASES = (
    (3, 1, 2, 4.0, HI | 3, False),
    (63, 16, 64, 1.5, HI | 63, False),
    (64, 17, 65, 50.0, HI | 64, False),
    (65, 1, 130, 4.0, 0, False),
    (65, 16, 2, 1.5, 2 ** 64 - 1, False),
    (129, 17, 130, 1.5, HI | 129, False),
    (129, 16, 64, 50.0, (7 << 32) | 5, True),
    (63, 1, 65, CYCLE, 2 ** 64 - 1, False),
    (64, 17, 130, CYCLE, 0, False),
    (65, 16, 130, CYCLE, HI | 65, True),
    (129, 1, 64, CYCLE, HI | 1290, False),
)


def case_nu(nu, S):
    """What a case hands over as nu: the value, or the (S,) cycle 1.5, 4, 50, 1.5, .."""
    return np.array([NUS[s % 3] for s in range(S)]) if nu == CYCLE else float(nu)


def case_id(c):
    return "n%d_k%d_S%d_nu%s" % (c[0], c[1], c[2], c[3])


_CACHE = {}


def _frozen(*arrays):
    for a in arrays:
        if a is not None and isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def case(c):
    """(n, S, A, y, theta, offset or None, seed, nu, t_rep, t_obs); computed once, never changed."""
    if c not in _CACHE:
        n, k, S, nu, seed, with_offset = c
        data_seed = 70000 + 1000 * k + 10 * n + S
        A, y, th = P.make_case(n, k, S, data_seed)
        off = 1.0 + 0.5 * np.random.default_rng(data_seed + 7).standard_normal(n) if with_offset else None
        nus = case_nu(nu, S)
        t_rep, t_obs = reference(A, y, th, seed, nus, offset=off)
        _CACHE[c] = (n, S) + _frozen(A, y, th, off) + (seed,) + _frozen(nus, t_rep, t_obs)
    return _CACHE[c]


BIASED_DELTA = 3.0
BIASED_NU = 4.0


def biased_case():
    """ppc_reference.make_biased(3.0) (200 x 2, 64 draws, the replicated mean 150 sd from mean(y))
    under t_4 noise, as case()."""
    key = ("biased",)
    if key not in _CACHE:
        A, y, th = P.make_biased(BIASED_DELTA)
        t_rep, t_obs = reference(A, y, th, P.BIASED_SEED, BIASED_NU)
        _CACHE[key] = (200, 64) + _frozen(A, y, th, None) + (P.BIASED_SEED, BIASED_NU) + _frozen(t_rep, t_obs)
    return _CACHE[key]


GROUPS = ("grid", "biased")


def group_cases(group):
    if group == "grid":
        for c in CASES:
            yield case(c)
    else:
        yield biased_case()


def accuracy_of(nus, n, S):
    """(n, S) float64: T_ACCURACY of every element's nu."""
    per_draw = np.array([T_ACCURACY[float(v)] for v in nu_of_draws(nus, S)])
    return np.broadcast_to(per_draw[None, :], (n, S))


def measured_floors(group):
    """(10,) float64, the rule of ppc_reference.measured_floors: per value of TEN over the group's
    cases, the larger of (a) the float64 reference's deviation from the long-double one and (b) the
    long-double reference with every z replaced by z (1 + d), |d| = T_ACCURACY of the element's nu
    with random signs, against the unperturbed one.  Neither involves the device."""
    worst = np.zeros(len(TEN))
    rng = np.random.default_rng(2025)
    for n, S, A, y, th, off, seed, nus, t_rep, t_obs in group_cases(group):
        ref = P.ten(t_rep, t_obs)
        f64 = P.ten(*reference(A, y, th, seed, nus, offset=off, dtype=np.float64))
        fac = 1 + accuracy_of(nus, n, S).astype(LD) * rng.choice([-1.0, 1.0], size=(n, S)).astype(LD)
        pert = P.ten(*reference(A, y, th, seed, nus, offset=off, z_factor=fac))
        worst = np.maximum(worst, np.maximum(P.deviation(f64, ref), P.deviation(pert, ref)))
    return worst


# measured_floors() of each group, rounded up to two digits; tests/test_ppc_t_host.py recomputes
# them and asserts that none exceeds its constant.  Measured in units of 1e-16 (the order of TEN):
#   grid     137   79.1  74.5  48.8  347    260   97.7  48.9  13.4  26.6
#   biased   1.13  2.05  9.62  1.03  10100  4450  16.2  12.0  9.85  3.45
# (grid: the nu = 1.5 cases set all but the last two -- T_ACCURACY is ten times Z_ACCURACY there, and
# one variate in a few hundred is beyond 30 sigma.  biased skew and kurt: |y_rep| / sd, as in
# ppc_reference.FLOORS.)
FLOORS = {
    "grid": (1.4e-14, 8.0e-15, 7.5e-15, 4.9e-15, 3.5e-14, 2.7e-14, 9.8e-15, 4.9e-15, 1.4e-15, 2.7e-15),
    "biased": (1.2e-16, 2.1e-16, 9.7e-16, 1.1e-16, 1.1e-12, 4.5e-13, 1.7e-15, 1.2e-15, 9.9e-16, 3.5e-16),
}


def bars(group):
    """{name of TEN: bar}: BAR_FACTOR x the floor, rounded up to one significant digit."""
    return {name: P.round_up_one_digit(BAR_FACTOR * f) for name, f in zip(TEN, FLOORS[group])}


# ---- the planted problem (tests/robust_reference.planted_problem(200, 3, ..)) -------------------------
def p_values_with_margin(t_rep, t_obs):
    """({name: p}, smallest compared margin) of a reference run."""
    return P.p_values(t_rep, t_obs), float(P.margins(t_rep, t_obs).min())
