"""The shared case list of the predictive leg's class tests (tests/test_predict_plan.py on the CPU,
tests/test_predict_classes_gpu.py on the GPU).

Exact draws: preds = 0, Vt_hat = 0, sigma = 1 and replayed noise make every draw the noise itself
(fma(z, 1, 0) = z), so each point's S draws are written exactly.  Points cycle through ROW_KINDS;
with the selection route each kind takes a known branch of predict_select_kernel (EXPECTED_ROUTE,
asserted on the inputs by tests/test_predict_plan.py with predict_reference.selection_route).
"""
from collections import namedtuple

import numpy as np

from predict_reference import requested_ranks

ROW_KINDS = ("normal", "ties8", "half", "far", "huge", "flat", "two", "subnormal")
# (of a row with S >= 2048 draws whose request includes a rank in the bulk)
EXPECTED_ROUTE = {"normal": "select", "ties8": "select", "half": "fallback", "far": "fallback",
                  "huge": "fallback", "flat": "flat", "two": "fallback", "subnormal": "unusable"}

Q6 = (2.5, 50, 97.5, 0, 100, 33.3)
COV21 = [float(p) for p in range(0, 101, 5)]
Q43 = tuple(float(x) for x in np.round(np.linspace(0, 100, 43), 1))
Q44 = tuple(float(x) for x in np.round(np.linspace(0, 100, 44), 1))
Q64 = tuple(float(x) for x in np.round(np.linspace(0, 100, 64), 2))
COV64 = [float(x) for x in np.round(np.linspace(0, 100, 64), 2)]

# both sides of every boundary of plan_predict_orderstat: the sort's powers of two, the switch to the
# selection at 2048, and every class of draws per thread (512 * 4 j)
S_SORT = (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2047)
S_SELECT = (2048, 2049, 4096, 4097, 6144, 6145, 8192, 8193, 10240, 10241, 12288, 12289, 14336,
            14337, 16384)

Case = namedtuple("Case", "name S M q cov")

CASES = (
    [Case(f"S{S}", S, 70, Q6, COV21) for S in S_SORT + S_SELECT]
    # 2 n_q + 2 n_cov = 128 still selects, 130 takes the sort as the primary route
    + [Case("S4096-ranks128", 4096, 70, Q43, COV21)]
    + [Case(f"S{S}-ranks130", S, 70, Q44, COV21) for S in (4096, 8192, 16384)]
    # the request limits of the C ABI
    + [Case(f"S{S}-q64-cov64", S, 70, Q64, COV64) for S in (64, 10000)]
    + [Case("S1000-cov-only", 1000, 70, (), COV21), Case("S6145-cov-only", 6145, 70, (), COV21),
       Case("S1000-q-only", 1000, 70, Q6, None), Case("S12289-q-only", 12289, 70, Q6, None)]
    # more points than workgroups: both point loops wrap (2048 and, behind the selection, 256)
    + [Case("S64-M2100", 64, 2100, Q6, COV21), Case("S2048-M2100", 2048, 2100, Q6, COV21)]
)
CASE_IDS = [c.name for c in CASES]
assert len(set(CASE_IDS)) == len(CASES)


def row_kind(p):
    return ROW_KINDS[p % len(ROW_KINDS)]


def make_row(kind, S, rng):
    """One point's S draws of the given kind, in random order."""
    z = rng.standard_normal(S)
    if kind == "ties8":        # every value 8 times: ties inside a resolvable bin
        z = rng.permutation(np.repeat(rng.standard_normal((S + 7) // 8), 8)[:S])
    elif kind == "half":       # half of the row one value
        z[rng.permutation(S)[: S // 2]] = 0.25
    elif kind == "far":        # one far draw stretches [min, max]
        z[rng.integers(S)] = 1e9
    elif kind == "huge":       # two draws at +-1e300
        i = rng.permutation(S)[:2]
        z[i[0]] = 1e300
        if S > 1:
            z[i[1]] = -1e300
    elif kind == "flat":       # every draw equal
        z[:] = -1.5
    elif kind == "two":        # two values only
        z = rng.integers(0, 2, S).astype(np.float64)
    elif kind == "subnormal":  # multiples of the smallest subnormal: a range too small to scale
        z = rng.integers(-1000, 1001, S) * 5e-324
    return z


def case_seed(case):
    return 1000003 * case.S + 101 * case.M + 7 * len(case.q) + (0 if case.cov is None else len(case.cov))


def case_inputs(case):
    """preds, theta, Vt, noise (S, M), truth (or None) of a case; deterministic."""
    rng = np.random.default_rng(case_seed(case))
    S, M, Km, k = case.S, case.M, 3, 2
    noise = np.empty((S, M))
    for p in range(M):
        noise[:, p] = make_row(row_kind(p), S, rng)
    truth = None
    if case.cov is not None:
        truth = rng.standard_normal(M)
        ranks = requested_ranks(S, (), case.cov)
        c = len(case.cov) // 2 + 1
        lo, hi = ranks[2 * c], ranks[2 * c + 1]
        srt = lambda p: np.sort(noise[:, p])
        # on a bound, and one ulp outside: of a row the selection resolves (kind "normal": points
        # 0, 8, ..) and of one it hands back (kind "half": points 2, 10, ..)
        for base in (0, 2):
            truth[base] = srt(base)[lo]
            truth[base + 8] = srt(base + 8)[hi]
            truth[base + 16] = np.nextafter(srt(base + 16)[hi], np.inf)
            truth[base + 24] = np.nextafter(srt(base + 24)[lo], -np.inf)
    return dict(preds=np.zeros((M, Km)), theta=np.column_stack([np.zeros((S, k)), np.ones(S)]),
                Vt=np.zeros((k, Km)), noise=noise, truth=truth)
