"""The reference of the Student-t power-scaling sensitivity (tests/sens_t_reference.py) without a
GPU: its log likelihood against an independent sum of t log densities, a table of one value against
the fixed-nu form, and where the prior of nu goes."""
import math

import numpy as np
import pytest

import sens_reference as SR
import sens_t_reference as ST

LD = np.longdouble


def _independent_loglik(A, y, theta, nus):
    """sum_i log t_nu((y_i - a_i . beta) / sigma) - N log sigma per draw: scipy's density if scipy is
    here, else lgamma-based terms."""
    k = A.shape[1]
    out = np.empty(theta.shape[0])
    try:
        from scipy import stats
        logpdf = lambda z, nu: stats.t.logpdf(z, nu)
    except ImportError:
        def logpdf(z, nu):
            c = math.lgamma((nu + 1) / 2) - math.lgamma(nu / 2) - 0.5 * math.log(nu * math.pi)
            return c - (nu + 1) / 2 * np.log1p(z * z / nu)
    for s, (th, nu) in enumerate(zip(theta, nus)):
        z = (y - A @ th[:k]) / th[k]
        out[s] = np.sum(logpdf(z, nu)) - len(y) * math.log(th[k])
    return out


def _tolerance(want, N, nus):
    """What the independent sum itself is good for: its constant is a difference of two float64
    lgamma, each a few ulp of its own size (about 55 at nu = 50), added N times; the rest is a few
    ulp of the sum."""
    eps = np.finfo(np.float64).eps
    lg = np.array([abs(math.lgamma((nu + 1) / 2)) + abs(math.lgamma(nu / 2)) + 1 for nu in nus])
    return 4 * eps * N * lg + 64 * eps * np.abs(want)


@pytest.mark.parametrize("nu", [1.5, 4.0, 50.0])
def test_loglik_is_the_sum_of_t_log_densities(nu):
    A, y, theta, prior, _ = SR.random_case(29, 3, 40, 5)
    y = y.copy()
    y[3] += 40.0
    ll = ST.log_densities_t(A, y, theta, prior, nu)[2]
    want = _independent_loglik(A, y, theta, np.full(40, nu))
    assert np.all(np.abs(ll - want) <= _tolerance(want, 29, np.full(40, nu)))
    # the long-double form agrees with the float64 one far inside what the GPU test allows
    ll_ld = ST.log_densities_t(A, y, theta, prior, nu, LD)[2]
    assert np.max(np.abs(ll_ld - ll) / np.abs(ll_ld)) < 1e-14


def test_loglik_with_a_nu_per_draw():
    A, y, theta, prior, _ = SR.random_case(17, 2, 30, 6)
    nus = np.array([1.5, 4.0, 50.0, 2.5])[np.arange(30) % 4]
    values, index = ST.nu_table(nus)
    assert list(values) == [1.5, 2.5, 4.0, 50.0] and np.array_equal(values[index], nus)
    ll = ST.log_densities_t(A, y, theta, prior, (values, index, None))[2]
    want = _independent_loglik(A, y, theta, nus)
    assert np.all(np.abs(ll - want) <= _tolerance(want, 17, nus))


@pytest.mark.parametrize("dtype", [np.float64, LD])
def test_a_table_of_one_value_is_the_fixed_nu_form_exactly(dtype):
    A, y, theta, prior, Vt = SR.random_case(12, 3, 50, 7, n_models=2)
    fixed = ST.log_densities_t(A, y, theta, prior, 4.0, dtype)
    table = ST.log_densities_t(A, y, theta, prior, (np.array([4.0]), np.zeros(50, dtype=int), None), dtype)
    for a, b in zip(fixed, table):
        assert a.dtype == dtype and np.array_equal(a, b)
    assert np.all(fixed[3] == 0)
    # lp_beta and lp_sigma2 are the Gaussian model's
    g = SR.log_densities(A, y, theta, prior, dtype)
    assert np.array_equal(fixed[0], g[0]) and np.array_equal(fixed[1], g[1])
    assert not np.array_equal(fixed[2], g[2])


def test_the_prior_of_nu_shifts_the_prior_and_nothing_else():
    A, y, theta, prior, _ = SR.random_case(12, 2, 60, 8)
    grid = np.array([1.5, 3.0, 6.0, 12.0])
    weight = np.array([1.0, 4.0, 2.0, 0.5])
    values, index = ST.nu_table(grid[np.arange(60) % 3])            # 12.0 is never drawn
    lpn = ST.log_prior_of(values, grid, weight)
    assert np.allclose(lpn, np.log(weight[:3] / 7.5))
    without = ST.log_densities_t(A, y, theta, prior, (values, index, None))
    with_p = ST.log_densities_t(A, y, theta, prior, (values, index, lpn))
    for j in range(3):
        assert np.array_equal(without[j], with_p[j])
    assert np.all(without[3] == 0) and np.array_equal(with_p[3], lpn[index])
    for name in ("likelihood", "prior_beta", "prior_sigma2"):
        assert np.array_equal(ST.component_vector(without, name), ST.component_vector(with_p, name))
    assert np.array_equal(ST.component_vector(with_p, "prior"),
                          ST.component_vector(without, "prior") + lpn[index])
    assert np.array_equal(ST.component_vector(with_p, "prior_nu"), lpn[index])


def test_bad_draws_have_no_log_density_and_the_nu_column_is_last():
    A, y, theta, prior, Vt = SR.random_case(9, 2, 30, 9, n_models=2)
    values, index = ST.nu_table(np.array([2.0, 5.0])[np.arange(30) % 2])
    nu = (values, index, np.log([0.25, 0.75]))
    bad = theta.copy()
    bad[4, 0] = np.nan
    bad[9, 2] = 0.0
    bad[11, 2] = np.inf
    lp = ST.log_densities_t(A, y, bad, prior, nu)
    for v in lp:
        assert np.isnan(v[[4, 9, 11]]).all() and np.isfinite(np.delete(v, [4, 9, 11])).all()
    X = ST.quantities_t(theta, Vt, nu)
    assert X.shape == (30, 2 + 1 + 2 + 1) and np.array_equal(X[:, -1], values[index])
    assert np.array_equal(X[:, :-1], SR.quantities(theta, Vt))
    assert ST.quantities_t(theta, Vt, 4.0).shape == (30, 5)
    r = ST.sensitivity(A, y, theta, prior, nu, Vt, components=ST.T_COMPONENTS)
    assert r["lp"].shape == (4, 30) and r["cjs"].shape == (5, 2, 6) and np.isfinite(r["cjs"]).all()
