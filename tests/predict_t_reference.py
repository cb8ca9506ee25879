"""The Student-t noise of the predictive kernel restated on the host.  TEST INFRASTRUCTURE ONLY.

numpy.longdouble and nothing of the kernel's text.  The ninth variate stream:

    z[s, p]   sqrt(nu_s expm1(-(2 / nu_s) log u1)) cos(2 pi u2), (u1, u2) the two uniforms of counter
              (e lo, e hi, STREAM_PRED_T, 0) under key = seed, e = p S + s: one counter per (point,
              draw), and the cosine half alone (ppc_t_reference.t_variate)

Arrays are (S, M) = (n_draws, n_points), the layout of the draws that predict() returns.  The CPU
build of the product's own student_t_variate is predict_t_host_build.py; T_ACCURACY (per nu, the
recorded worst case of that build against long double) is ppc_t_reference's.
"""
import functools

import numpy as np

import ppc_t_reference as T
import rng_reference as G

LD = np.longdouble
STREAM_PRED_T = 0x50524554         # "PRET"
NUS = T.NUS
T_ACCURACY = T.T_ACCURACY
CYCLE = "cycle"
# the seeds of the statistical tests (tests/test_predict_t_host.py: the restatement passes them on the
# CPU) and of the GPU tests
SEEDS = (11, 2 ** 32 + 7)


def counter_index(S, M):
    """(S, M) uint64: e = p S + s of entry (draw s, point p)."""
    s = np.arange(S, dtype=np.uint64)[:, None]
    p = np.arange(M, dtype=np.uint64)[None, :]
    return p * np.uint64(S) + s


@functools.lru_cache(maxsize=4)
def uniforms(seed, S, M):
    """(u1, u2), both (S, M) float64; computed once per (seed, shape), never changed."""
    u1, u2 = G.pair_uniforms(G.stream_words(seed, counter_index(S, M), STREAM_PRED_T))
    u1.setflags(write=False)
    u2.setflags(write=False)
    return u1, u2


def nu_of_draws(nu, S):
    """(S,) float64: one nu for all draws, the cycle 1.5, 4, 50, 1.5, .., or the given one per draw."""
    if isinstance(nu, str) and nu == CYCLE:
        return np.array([NUS[s % 3] for s in range(S)])
    return T.nu_of_draws(nu, S)


def call_nu(nu, S):
    """The keyword of Context.predict for a case's nu: {"nu": value} or {"nu_draws": (S,)}."""
    if isinstance(nu, str) or np.ndim(nu) != 0:
        return {"nu_draws": nu_of_draws(nu, S)}
    return {"nu": float(nu)}


def noise(seed, S, M, nu):
    """(S, M) long double: the restated noise matrix."""
    u1, u2 = uniforms(seed, S, M)
    return T.t_variate(u1, u2, nu_of_draws(nu, S)[:, None])[0]


def accuracy(nu, S):
    """(S, 1) float64: T_ACCURACY of every draw's nu."""
    return np.array([T_ACCURACY[float(v)] for v in nu_of_draws(nu, S)])[:, None]
