"""The references of tests/diag_exact_reference.py alone, on the CPU, for every input the class tests
of the diagnostics kernels use (tests/diag_cases.py).  Each bound is sharp: an autocovariance's at
most SHARP = 1e-11 of its column's a(0), an M2's the same fraction of the M2, a mean's of the
half-chain's sd; and honest: numpy's own float64 evaluation of the same sums (another correct order
of the same operations) lies inside it."""
import numpy as np
import pytest

import diag_cases as dc
import diag_exact_reference as X

SHARP = 1e-11


def check(ref, x, burn, cols, t0, nl):
    n = ref["n"]
    P = ref["shift"].shape[0]
    cols = np.arange(P) if cols is None else cols
    a0 = X.exact(x, burn, cols, 0, 1)["acov"][:, :1] if t0 else ref["acov"][:, :1]
    live = t0 + np.arange(nl) < n
    assert np.all(a0 > 0)
    assert np.all(ref["dacov"][:, live] > 0) and np.all(ref["dacov"][:, live] <= SHARP * a0)
    assert not ref["dacov"][:, ~live].any() and not ref["acov"][:, ~live].any()
    assert np.all(ref["dm2"] > 0) and np.all(ref["dm2"] <= SHARP * ref["seq_m2"])
    assert np.all(ref["dmean"] > 0) and np.all(ref["dmean"] <= SHARP * np.sqrt(ref["seq_m2"] / n))
    got = X.float64_evaluation(x, burn, cols, t0, nl)
    ratios = {k: X.worst_ratio(got[k], ref[k], ref[b])
              for k, b in (("seq_mean", "dmean"), ("seq_m2", "dm2"), ("acov", "dacov"))}
    sharp = float(np.max(ref["dacov"][:, live] / a0))
    print("n = %d, q = %d: worst bound / a(0) = %.2e, float64 ratios %s" % (n, ref["q"], sharp, ratios))
    assert max(ratios.values()) <= 1.0, ratios
    assert ratios["acov"] > 0.0        # (and the float64 sums are not the reference itself)


@pytest.mark.parametrize("tag", list(dc.ACOV_CASES))
def test_acov_bounds_are_sharp_and_hold_for_numpy(tag):
    check(dc.acov_reference(tag), *dc.acov_call(tag))


@pytest.mark.parametrize("key", list(dc.MOMENT_CASES), ids=dc.moment_id)
def test_moment_bounds_are_sharp_and_hold_for_numpy(key):
    C, T, burn, P = key
    check(dc.moment_reference(key), dc.samples(C, T, P), burn, None, 0, 1)


def test_inputs_are_what_the_table_promises():
    x = dc.samples(8, 2200, 64)
    sd = x.std(axis=(0, 1))
    assert abs(x[:, :, 32].mean() - 1e4) < 1.0 and 0.5e-2 < sd[32] < 2e-2
    off = np.abs(x.mean(1) - x.mean((0, 1))) / sd
    assert off.max() < 2.0                      # half an sd of offset plus the chain's own wander
    # lag-1 autocorrelation by column: phi = 0, 0.5, 0.9, 0.99 in turn
    ref = X.exact(x, 0, None, 0, 2)["acov"].astype(np.float64)
    rho1 = ref[:, 1] / ref[:, 0]
    for r, phi in enumerate(dc.PHIS):
        assert np.all(np.abs(rho1[r::4] - phi) < 0.12), (phi, rho1[r::4])


def test_reference_against_exact_rationals():
    """On the smallest input the longdouble values are the exact ones to 2^-58."""
    from fractions import Fraction as Fr
    x, burn, cols, t0, nl = dc.acov_call("A2")
    ref = dc.acov_reference("A2")
    halves, _, shift = X.split(x, burn)
    M, n, _ = halves.shape
    for j in (0, 2):
        for t in (0, 1, 8):
            tot = Fr(0)
            for m in range(M):
                y = [Fr(float(v)) - Fr(float(shift[j])) for v in halves[m, :, j]]
                mu = sum(y) / n
                tot += sum((y[i] - mu) * (y[i + t] - mu) for i in range(n - t)) / n
            tot /= M
            v = ref["acov"][j, t]
            hi, lo = float(v), float(v - X.LD(float(v)))
            a0 = float(ref["acov"][j, 0])
            assert abs(Fr(hi) + Fr(lo) - tot) <= Fr(a0) * Fr(1, 2 ** 58), (j, t)


def test_a_wrong_sum_is_far_outside_the_bounds():
    """What the bounds are for: a half-chain left out of the average, a tile's rows dropped, or a
    mean taken from the neighbouring half-chain is 10^8 bounds away or more."""
    x, burn, cols, t0, nl = dc.acov_call("B")
    ref = dc.acov_reference("B")
    halves, _, shift = X.split(x, burn)
    M, n, P = halves.shape
    d = (halves - shift) - (halves - shift).mean(1)[:, None, :]

    def acov_of(dd, rows, seqs):
        out = np.zeros((P, nl))
        for t in range(nl):
            hi = min(rows, n - t)
            out[:, t] = (dd[seqs, :hi] * dd[seqs, t:t + hi]).sum(1).sum(0) / n / M
        return out

    right = acov_of(d, n, slice(None))
    assert X.worst_ratio(right, ref["acov"], ref["dacov"]) <= 1.0
    assert X.worst_ratio(acov_of(d, n, slice(1, None)), ref["acov"], ref["dacov"]) > 1e8
    assert X.worst_ratio(acov_of(d, 128, slice(None)), ref["acov"], ref["dacov"]) > 1e8
    shifted = (halves - shift) - np.roll((halves - shift).mean(1), 1, axis=0)[:, None, :]
    assert X.worst_ratio(acov_of(shifted, n, slice(None)), ref["acov"], ref["dacov"]) > 1e8
