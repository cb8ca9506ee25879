"""CPU checks of the per-draw-nu score reference (tests/tscore_nu_reference.py): one value for all
draws is the scalar reference, and the rounding floors its bars are formed from."""
import numpy as np

import tscore_nu_reference as TV
import tscore_reference as T


def test_one_value_is_the_scalar_reference():
    for k, n, S in TV.SHAPES:
        A, y, th = T.shape_case(k, n, S)
        for nu in T.NUS:
            a, b = TV.pointwise(A, y, th, np.full(S, nu)), T.pointwise(A, y, th, nu)
            la, lb = TV.loo_pointwise(A, y, th, np.full(S, nu)), T.loo_pointwise(A, y, th, nu)
            assert all(np.array_equal(a[key], b[key]) for key in b)
            assert all(np.array_equal(la[key], lb[key]) for key in lb)


def test_cycling_nu_is_not_any_single_nu():
    k, n, S = TV.SHAPES[-1]
    A, y, th = T.shape_case(k, n, S)
    ref = TV.reference(k, n, S)[0]
    assert set(TV.cycling_nu(S)) == set(TV.CYCLE)
    for nu in TV.CYCLE:
        assert np.max(np.abs(ref["lppd"] - T.pointwise(A, y, th, nu)["lppd"])) > 1e-3
    # column s of the matrix is the scalar density at nu_s
    ll = TV.loglik_tv(A, y, th, TV.cycling_nu(S))
    for j, nu in enumerate(TV.CYCLE):
        assert np.array_equal(ll[:, j::3], T.loglik_t(A, y, th[j::3], nu))


def test_reference_rounding_floor():
    """float64 against long double on the cases of test_tscore_nu_gpu.py: the floors the bars are
    100 x of.  Measured: elpd_loo_i 8.95e-16, pareto_k 3.33e-15 (lppd 9.9e-16, p_waic_i 6.0e-16,
    mean_ll_i 2.8e-16, under the fixed 1e-11 bars by four orders)."""
    worst = {}
    for shape in TV.SHAPES:
        d = T.deviations(TV.reference(*shape), *TV.reference(*shape, np.longdouble))
        for key, v in d.items():
            worst[key] = max(worst.get(key, 0.0), v)
    print(worst)
    assert worst["elpd_loo"] <= TV.FLOOR_ELPD and worst["pareto_k"] <= TV.FLOOR_K
    assert worst["elpd_loo"] >= 0.5 * TV.FLOOR_ELPD and worst["pareto_k"] >= 0.5 * TV.FLOOR_K
    assert max(worst["lppd"], worst["p_waic"], worst["mean_ll"]) <= 0.01 * TV.BAR_LPPD
