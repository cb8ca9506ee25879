"""Shapes and inputs of the chain-diagnostics class tests (kernels_diag.hip through
bmc_chain_autocov), shared by the CPU tests that pin each shape's launch plan and check the exact
references (test_diag_plan.py, test_diag_reference_host.py) and by the GPU tests that run them
(test_diag_classes_gpu.py).  n = (T - burn) // 2; the largest input is 22 MB.

ACOV_CASES: tag -> the call and the plan it must get from acov_plan (bmc_diag_plan.h):
column groups ncc, lag chunks nlc, sequence groups MG of spg half-chains, row splits S of rps rows.
  A1  the smallest legal input (n = 4): lags 4..63 are exactly 0
  A2  T' odd (the middle sequences exist), n < 64
  B   a partial second tile, one tile per split
  C   n = 150, first lag > 0 (the `as` tile is staged from memory), lags 150..191 exactly 0, 4 live
      columns in the last column group
  D   two tiles per split, nine tiles in all; the last split is one partial tile of 76 rows
  D0  D's plan from lag 0: at lags >= 192 the 76 rows of D's last split pair with nothing (i + t >= n),
      here they do, and lag chunk 0 takes the copy path while chunks 1..3 stage from memory
  E   spg = 3 with the last group clipped to 2 half-chains
  F   spg = 2 and three tiles in the one split
  F0  F's plan from lag 0: at lags >= 192 only rows i < 108 of F's first tile pair with anything,
      here all three tiles do
  G   at least 2048 (column group, lag chunk) units: MG = 1, spg = 2C; both staging paths in one
      launch, two tiles, lags >= 130 exactly 0
  H   the cols indirection: 21 of 40 columns, shuffled and non-contiguous

MOMENT_CASES: (C, T, burn, P) -> (column chunks ncc, row splits S, rows per split rps) of
moment_plan; called with one lag.  The ACOV_CASES' own moments are checked as well."""
import functools

import numpy as np

PHIS = (0.0, 0.5, 0.9, 0.99)

ACOV_CASES = {
    "A1": dict(shape=(1, 8, 0, 1), lags=(0, 64), plan=(1, 1, 2, 1, 1, 128)),
    "A2": dict(shape=(3, 19, 0, 5), lags=(0, 9), plan=(1, 1, 6, 1, 1, 128)),
    "B": dict(shape=(2, 260, 0, 3), lags=(0, 64), plan=(1, 1, 4, 1, 2, 128)),
    "C": dict(shape=(2, 310, 10, 20), lags=(64, 128), plan=(2, 2, 4, 1, 2, 128)),
    "D": dict(shape=(8, 2200, 0, 64), lags=(192, 256), plan=(4, 4, 16, 1, 5, 256)),
    "D0": dict(shape=(8, 2200, 0, 64), lags=(0, 256), plan=(4, 4, 16, 1, 5, 256)),
    "E": dict(shape=(100, 80, 0, 336), lags=(0, 40), plan=(21, 1, 67, 3, 1, 128)),
    "F": dict(shape=(32, 600, 0, 144), lags=(192, 256), plan=(9, 4, 32, 2, 1, 384)),
    "F0": dict(shape=(32, 600, 0, 144), lags=(0, 256), plan=(9, 4, 32, 2, 1, 384)),
    "G": dict(shape=(1, 260, 0, 4096), lags=(0, 512), plan=(256, 8, 1, 2, 1, 256)),
    "H": dict(shape=(3, 600, 0, 40), lags=(0, 64), n_active=21, plan=(2, 1, 6, 1, 3, 128)),
}

MOMENT_CASES = {
    (2, 515, 0, 130): (3, 2, 129),     # T' odd, last split 128 rows, a partial third column chunk
    (1, 2051, 1, 2): (1, 5, 205),
    (600, 40, 0, 4): (1, 1, 20),       # 1200 sequences: one split whatever n
}
# n = 15 .. 33 on both sides of the 16-row unrolled loop (a wave's rows: w, w + 4, ...)
MOMENT_CASES.update({(1, T, 0, 3): (1, 1, T // 2) for T in (30, 32, 34, 38, 62, 66)})


def moment_id(key):
    return "x".join(str(v) for v in key)


@functools.lru_cache(maxsize=None)
def samples(C, T, P):
    """AR(1) chains (diag_reference.ar1) with phi = 0, 0.5, 0.9, 0.99 by column, column P // 2 at
    loc 1e4 and scale 1e-2, and every chain's mean offset by up to half a marginal sd.  Shared
    between tests: read-only."""
    import diag_reference as R
    rng = np.random.Generator(np.random.PCG64([C, T, P]))
    phi = np.asarray(PHIS)[np.arange(P) % len(PHIS)]
    loc, scale = np.zeros(P), np.ones(P)
    loc[P // 2], scale[P // 2] = 1e4, 1e-2
    x = R.ar1(rng, C, T, P, phi, loc=loc, scale=scale)
    x += scale * rng.uniform(-0.5, 0.5, (C, 1, P))
    x.setflags(write=False)
    return x


def acov_call(tag):
    """(samples, burn, cols or None, first_lag, n_lags) of an ACOV_CASES row."""
    c = ACOV_CASES[tag]
    C, T, burn, P = c["shape"]
    cols = None
    if "n_active" in c:
        cols = np.random.Generator(np.random.PCG64(7)).permutation(P)[:c["n_active"]].astype(np.int32)
        assert np.any(np.diff(np.sort(cols)) > 1) and np.any(np.diff(cols) < 0)
    return samples(C, T, P), burn, cols, c["lags"][0], c["lags"][1]


@functools.lru_cache(maxsize=None)
def acov_reference(tag):
    """diag_exact_reference.exact of the row, computed once."""
    import diag_exact_reference as X
    x, burn, cols, t0, nl = acov_call(tag)
    return X.exact(x, burn, cols, t0, nl)


@functools.lru_cache(maxsize=None)
def moment_reference(key):
    import diag_exact_reference as X
    C, T, burn, P = key
    return X.exact(samples(C, T, P), burn, None, 0, 1)
