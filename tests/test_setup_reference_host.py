"""The references of tests/setup_reference.py alone, on the CPU, for every input the GPU tests of
the set-up kernels use (tests/setup_cases.py): each error bound is sharp -- at most STEP_TOL = 1e-12
of the result's scale, the bar rss and Gram already answer to -- and honest: numpy's own float64
evaluation of the same quantity (another correct order of the same operations) lies inside it."""
import numpy as np
import pytest

import setup_cases as sc
import setup_reference as R

STEP_TOL = 1e-12


@pytest.mark.parametrize("key", list(sc.RSS_CASES) + [("f32", 777, 6)], ids=sc.case_id)
def test_rss_bound_is_sharp_and_holds_for_numpy(key):
    y, X, B = sc.rss_inputs(*key)
    val, bound = sc.rss_reference(*key)
    assert val.shape == bound.shape == (9,)
    assert np.all(bound > 0) and np.all(bound <= STEP_TOL * val)
    yd, Xd = y.astype(np.float64), X.astype(np.float64)
    got = [np.sum((yd - Xd @ b) ** 2) for b in B] + [yd @ yd]
    assert R.worst_ratio(got, val, bound) <= 1.0
    # the values are of the size the inputs promise: O(1) residuals
    assert np.all(val > 0.5 * len(y)) and np.all(val < 4.0 * len(y))


def test_rss_reference_against_exact_rationals():
    """On a problem small enough for exact arithmetic the reference is the exact value to 2^-60."""
    from fractions import Fraction
    y, X, B = sc.rss_inputs("f64", 63, 2)
    val, _ = sc.rss_reference("f64", 63, 2)
    for i in (0, 7):
        exact = sum((Fraction(float(yi)) - sum(Fraction(float(x)) * Fraction(float(b)) for x, b in zip(xi, B[i]))) ** 2
                    for yi, xi in zip(y, X))
        hi, lo = float(val[i]), float(val[i] - R.LD(float(val[i])))     # the longdouble, in two floats
        assert abs(Fraction(hi) + Fraction(lo) - exact) <= exact * Fraction(1, 2 ** 60)


@pytest.mark.parametrize("key", list(sc.ORTHO_CASES), ids=sc.case_id)
def test_ortho_bounds_are_sharp_and_hold_for_numpy(key):
    n, km, k, _ = key
    F, truth = sc.ortho_inputs(n, km)
    mu64 = F.mean(1)
    Fc64 = F - mu64[:, None]
    # a stand-in for the device's answer: any orthonormal Vt and its S exercise the same algebra
    _, S, Vt = np.linalg.svd(Fc64, full_matrices=False)
    S, Vt = S[:k], Vt[:k]
    ref = R.ortho_ref(F, truth, Vt, S)
    for name, bname in (("mu", "dmu"), ("yc", "dyc"), ("U", "dU")):
        scale = np.max(np.abs(ref[name]))
        assert np.all(ref[bname] > 0) and np.max(ref[bname]) <= STEP_TOL * scale, name
    assert ref["U"].shape == (n, k)
    assert R.worst_ratio(mu64, ref["mu"], ref["dmu"]) <= 1.0
    assert R.worst_ratio(truth - mu64, ref["yc"], ref["dyc"]) <= 1.0
    assert R.worst_ratio(Fc64 @ ref["W"], ref["U"], ref["dU"]) <= 1.0
    # and U is what it should be: orthonormal columns
    assert np.abs((Fc64 @ ref["W"]).T @ (Fc64 @ ref["W"]) - np.eye(k)).max() < 1e-9


def test_a_wrong_column_is_far_outside_the_bounds():
    """What the bounds are for: one column of U taken from its neighbour's coefficients, or one row
    of a panel dropped from rss, is 10^10 bounds away."""
    F, truth = sc.ortho_inputs(577, 10)
    Fc = F - F.mean(1)[:, None]
    _, S, Vt = np.linalg.svd(Fc, full_matrices=False)
    ref = R.ortho_ref(F, truth, Vt[:9], S[:9])
    wrong = Fc @ ref["W"]
    wrong[:, 8] = wrong[:, 7]
    assert R.worst_ratio(wrong, ref["U"], ref["dU"]) > 1e10
    y, X, B = sc.rss_inputs("f64", 1237, 5)
    val, bound = sc.rss_reference("f64", 1237, 5)
    short = np.sum((y[:-1] - X[:-1] @ B[0]) ** 2)
    assert R.worst_ratio([short], val[:1], bound[:1]) > 1e10
