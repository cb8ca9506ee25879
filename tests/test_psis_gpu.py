"""PSIS-LOO on the MI355X (kernels_loo.hip, pybmc_amd.scoring.psis_loo) against the dense numpy
reference of tests/psis_reference.py.

Tolerances are 100 x the rounding floor of the float64 reference against np.longdouble, measured
on these very cases by test_psis_host.py::test_reference_rounding_floor (the margin WAIC uses, for
the same reasons: the device's exp / log / log1p are not correctly rounded, the MFMA and the
reductions sum in another order):

    elpd_loo_i   floor 3.04e-15 relative to max(1, |ref|) (c1)   -> bar 3.1e-13
    pareto_k     floor 1.18e-12 absolute (tight)                 -> bar 1.2e-10
    lppd         the existing 1e-11 bar of test_scoring_gpu.py

Points whose reference pareto_k exceeds 1 (the 40-sigma outliers, k-hat 9 to 20: PSIS itself calls
such an estimate meaningless) have their own measured floor 6.89e-16 (c1) -> bar 6.9e-14 for
elpd_loo_i, and pareto_k is held to "> 0.7 and finite like the reference".  No point is left out.

Measured on the MI355X over all cases of this file: elpd_loo_i 5.3e-15 (points with k > 1:
2.3e-15), pareto_k 1.2e-13, lppd 2.6e-15."""
import numpy as np
import pytest

import psis_reference as P
import score_reference as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

FLOOR_ELPD, FLOOR_K, FLOOR_ELPD_BIG = 3.1e-15, 1.2e-12, 6.9e-16
TOL_ELPD, TOL_K, TOL_ELPD_BIG, TOL_LPPD = 100 * FLOOR_ELPD, 100 * FLOOR_K, 100 * FLOOR_ELPD_BIG, 1e-11


def check(got, ref, tag=""):
    """Every point of the case against the reference; prints the figures before it asserts."""
    rk = np.asarray(ref["pareto_k"], dtype=np.float64)
    gk = np.asarray(got["pareto_k"], dtype=np.float64)
    re_ = np.asarray(ref["elpd_loo"], dtype=np.float64)
    assert np.isfinite(re_).all() and not np.isnan(rk).any(), tag
    big = rk > 1
    d_e = np.abs(got["elpd_loo"] - re_) / np.maximum(1.0, np.abs(re_))
    d_l = np.abs(got["lppd"] - ref["lppd"]) / np.maximum(1.0, np.abs(ref["lppd"]))
    same_inf = np.isinf(rk) == np.isinf(gk)
    d_k = np.where(np.isinf(rk) | np.isinf(gk), 0.0, np.abs(gk - rk))
    print(f"{tag}: elpd {d_e[~big].max() if (~big).any() else 0:.3e} (k > 1: "
          f"{d_e[big].max() if big.any() else 0:.3e}, {int(big.sum())} points)  "
          f"k {d_k[~big].max() if (~big).any() else 0:.3e}  lppd {d_l.max():.3e}  "
          f"inf agree {bool(same_inf.all())}")
    assert same_inf.all(), tag
    assert not np.isnan(gk).any() and np.isfinite(got["elpd_loo"]).all(), tag
    assert d_l.max() <= TOL_LPPD, tag
    assert np.all(d_e[~big] <= TOL_ELPD), tag
    assert np.all(d_k[~big] <= TOL_K), tag
    assert np.all(d_e[big] <= TOL_ELPD_BIG), tag
    assert np.all(gk[big] > P.HIGH_K), tag


def raw(A, y, th, **kw):
    """elpd_loo, pareto_k, lppd as check() wants them."""
    from pybmc_amd import psis_loo
    out = psis_loo(A, y, th, **kw)
    assert np.array_equal(out["p_loo_i"], out["lppd"] - out["elpd_loo_i"], equal_nan=True)
    return {"elpd_loo": out["elpd_loo_i"], "pareto_k": out["pareto_k"], "lppd": out["lppd"]}, out


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_synthetic_cases_with_a_far_outlier(name):
    A, y, th = R.synth_case(name)
    ref = P.pointwise(A, y, th)
    got, out = raw(A, y, th)
    check(got, ref, name)
    assert out["pareto_k"][0] > P.HIGH_K and out["n_high_k"] >= 1
    assert out["n_high_k"] == int(np.sum(ref["pareto_k"] > P.HIGH_K))
    for key, v in P.loo_summary(ref, len(th)).items():
        assert out[key] == pytest.approx(v, rel=1e-9), key


@pytest.mark.parametrize("name", P.GOLDEN)
def test_golden_chains_as_draws(name):
    g = load_golden(name)
    A, y, th = np.asarray(g["X"], dtype=np.float64), g["y"], g["samples"]
    ref = P.pointwise(A, y, th)
    got, out = raw(np.asfortranarray(A), y, th)
    check(got, ref, name)
    for key, v in P.loo_summary(ref, len(th)).items():
        assert out[key] == pytest.approx(v, rel=1e-9), key
    if name == "gibbs_ortho629x3":
        assert out["n_high_k"] == 0


@pytest.mark.parametrize("k", R.SHAPE_K)
def test_shapes_on_both_sides_of_every_rule(k):
    """k across the MFMA step and the slab; points across the 64-wide tile; draws below and at the
    M >= 5 rule (24, 25), lanes without a draw, several splits (4097: the only S above the
    candidate cap, so the radix select runs); both layouts, lda and ldt wider than the rows."""
    from pybmc_amd import _lib
    ctx = _lib.default_context(0)
    for case, n, S, (A, y, th) in P.shape_cases(k):
        ref = P.pointwise(A, y, th)
        pad_a, pad_t = (case % 3) * 2, (case % 2) * 3
        if case % 2:
            buf = np.full((k, n + pad_a), np.nan)
            buf[:, :n] = A.T
            lda, layout = n + pad_a, _lib.BMC_COL_MAJOR
        else:
            buf = np.full((n, k + pad_a), np.nan)
            buf[:, :k] = A
            lda, layout = k + pad_a, _lib.BMC_ROW_MAJOR
        tb = np.full((S, k + 1 + pad_t), np.nan)
        tb[:, :k + 1] = th
        with ctx.lock:
            got = ctx.psis_loo(buf, n, k, lda, layout, y, tb, S, k + 1 + pad_t)
        if S < 25:
            assert np.isinf(got["pareto_k"]).all()
        check(got, ref, f"k={k} n={n} S={S} layout={layout} lda={lda} ldt={k + 1 + pad_t}")


def test_pooling_burn_thin_and_device_tensors():
    import torch
    A, y, th = R.random_case(130, 6, 4 * 3000, 33)
    chains = th.reshape(4, 3000, 7)
    for burn, thin in ((0, 1), (100, 1), (37, 3)):
        ref = P.pointwise(A, y, R.pool(chains, burn, thin))
        got, out = raw(A, y, chains, burn=burn, thin=thin)
        check(got, ref, f"numpy burn={burn} thin={thin}")
        assert out["n_draws"] == len(R.pool(chains, burn, thin))
        td = torch.as_tensor(chains, device="cuda:0")
        got_t, _ = raw(A, y, td, burn=burn, thin=thin)
        check(got_t, ref, f"torch burn={burn} thin={thin}")
        for key in got:
            assert np.array_equal(got[key], got_t[key]), key
    ref = P.pointwise(A, y, chains[2, 50::4])
    check(raw(A, y, chains[2], burn=50, thin=4)[0], ref, "one chain")
    check(raw(A, y, torch.as_tensor(chains[2], device="cuda:0"), burn=50, thin=4)[0], ref, "one chain, torch")


# ---- adversarial rows for the select --------------------------------------------------------------
def test_identical_draws_are_not_smoothed():
    A, y, th = R.random_case(300, 7, 2, 5)
    th = np.repeat(th[:1], 6001, axis=0)     # S above the cap: the select sees one value per point
    got, out = raw(A, y, th)
    assert np.isinf(got["pareto_k"]).all() and (got["pareto_k"] > 0).all()
    assert np.all(np.abs(got["elpd_loo"] - got["lppd"]) <= 1e-13 * np.maximum(1, np.abs(got["lppd"])))
    check(got, P.pointwise(A, y, th), "identical draws")


def test_a_run_of_ties_across_the_cutoff():
    """One draw repeated S / 2 times, its coefficients moved away from the fit so that it is among
    the worst draws of many points: there the cutoff falls inside the run of ties (asserted
    below).  The same draws permuted: the result depends on the values alone."""
    A, y, th = R.random_case(200, 5, 9000, 77)
    rng = np.random.default_rng(3)
    rep = th[0].copy()
    rep[:5] += 0.5                           # far from the fit: low ll at most points
    t2 = th.copy()
    t2[rng.permutation(9000)[:4500]] = rep
    ref = P.pointwise(A, y, t2)
    got, _ = raw(A, y, t2)
    check(got, ref, "S/2 ties")
    perm = rng.permutation(9000)
    got_p, _ = raw(A, y, t2[perm])
    check(got_p, ref, "S/2 ties, permuted")
    M = P.tail_length(9000)
    ll = R.loglik(A, y, t2)
    inside = [(np.sort(row)[M] == np.sort(row)[M - 1]) for row in ll]
    assert sum(inside) >= 20                 # the cutoff does fall inside a run of ties


def test_values_within_a_few_ulp_and_a_wide_span():
    """A point whose ll differ only in the last bits (a_i = 0: ll = -log sigma_s - const, sigma
    within a few ulp): the select has to fix nearly all 64 key bits; and the 600-unit span of the
    outlier next to it."""
    A, y, th = R.synth_case("c1")
    A = A.copy()
    A[5] = 0.0
    th = th.copy()[:9000]
    th[:, -1] = 0.5 * (1 + np.arange(9000) % 7 * 2.0 ** -51)
    ref = P.pointwise(A, y, th)
    assert ref["lppd"][0] < -600
    ll5 = R.loglik(A[5:6], y[5:6], th)[0]
    assert 1 < len(np.unique(ll5)) <= 8 and np.ptp(ll5) < 1e-14
    got, _ = raw(A, y, th)
    check(got, ref, "few ulp + wide span")


def test_two_calls_return_the_same_bits():
    import torch
    A, y, th = R.random_case(500, 12, 9000, 21)
    a, _ = raw(A, y, th)
    b, _ = raw(A, y, th)
    c, _ = raw(A, y, torch.as_tensor(th, device="cuda:0"))
    for key in a:
        assert np.array_equal(a[key], b[key]), key
        assert np.array_equal(a[key], c[key]), key
    from pybmc_amd import pointwise_log_likelihood
    assert np.array_equal(a["lppd"], pointwise_log_likelihood(A, y, th)["lppd"])
    check(a, P.pointwise(A, y, th), "determinism case")


def test_non_finite_values_are_values():
    A, y, th = R.random_case(200, 5, 7000, 9)
    ref = P.pointwise(A, y, th)
    keys = ("elpd_loo", "pareto_k", "lppd")
    for bad in (np.nan, np.inf):
        A2 = A.copy()
        A2[17, 2] = bad
        got, _ = raw(A2, y, th)
        ok = np.arange(200) != 17
        for key in keys:
            assert np.isnan(got[key][17]), (key, bad)
            np.testing.assert_allclose(got[key][ok], ref[key][ok], rtol=1e-9)
        y2 = y.copy()
        y2[130] = bad
        got, _ = raw(A, y2, th)
        ok = np.arange(200) != 130
        for key in keys:
            assert np.isnan(got[key][130]), (key, bad)
            np.testing.assert_allclose(got[key][ok], ref[key][ok], rtol=1e-9)
    for row, col, val in ((333, 1, np.nan), (6999, 5, 0.0), (0, 5, -0.3), (64, 5, np.nan)):
        t2 = th.copy()
        t2[row, col] = val
        got, _ = raw(A, y, t2)
        for key in keys:
            assert np.isnan(got[key]).all(), (key, row, col, val)


def test_c_abi_refuses_bad_arguments():
    from pybmc_amd import _lib
    ctx = _lib.default_context(0)
    A, y, th = R.random_case(10, 3, 20, 1)
    for args, msg in (((A, 10, 3, 3, 0, y, th, 1, 4), "n_draws"), ((A, 10, 3, 2, 0, y, th, 20, 4), "lda"),
                      ((A, 10, 3, 3, 0, y, th, 20, 3), "ldt"), ((A, 0, 3, 3, 0, y, th, 20, 4), "n_points"),
                      ((A, 10, 0, 3, 0, y, th, 20, 4), "k must"), ((A, 10, 3, 3, 2, y, th, 20, 4), "layout")):
        with pytest.raises(ValueError, match=msg):
            ctx.psis_loo(*args)


# ---- the BayesianModelCombination surface ---------------------------------------------------------
def _fit(kept, chains):
    from pybmc_amd import BayesianModelCombination
    train, models = R.three_component_frame(400, seed=1)
    b = BayesianModelCombination(models, {"p": train}, truth_column_name="truth")
    with pytest.raises(ValueError, match="orthogonalize"):
        b.loo()
    b.orthogonalize("p", train, components_kept=kept, method="svd")
    b.train({"iterations": 3000, "burn": 500, "n_chains": chains, "seeds": list(range(1, chains + 1))})
    return b


@pytest.mark.parametrize("chains", [1, 4])
def test_bmc_loo_equals_psis_loo(chains):
    from pybmc_amd import psis_loo
    b = _fit(3, chains)
    a = b.loo()
    s = np.asarray(b.samples).reshape(chains, -1, 4)
    w = psis_loo(b.U_hat, np.asarray(b.centered_experiment_train, dtype=np.float64), s)
    for key, v in w.items():
        assert np.array_equal(a[key], v), key
    assert a["n_draws"] == s.shape[0] * s.shape[1] and a["n_points"] == 400
    ref = P.pointwise(b.U_hat, b.centered_experiment_train, s.reshape(-1, 4))
    check({"elpd_loo": a["elpd_loo_i"], "pareto_k": a["pareto_k"], "lppd": a["lppd"]}, ref, "bmc.loo")
    ab = b.loo(burn=200)
    refb = P.pointwise(b.U_hat, b.centered_experiment_train, R.pool(s, 200))
    check({"elpd_loo": ab["elpd_loo_i"], "pareto_k": ab["pareto_k"], "lppd": ab["lppd"]}, refb, "bmc.loo(burn)")
    assert 2.0 < a["p_loo"] < 6.0          # k + 1 = 4 parameters


def test_elpd_loo_ranks_components_kept_like_held_out_data():
    val, _ = R.three_component_frame(200, seed=2)
    b1, b3 = _fit(1, 2), _fit(3, 2)
    l1, l3 = b1.loo(), b3.loo()
    e1, e3 = b1.log_predictive_density(val), b3.log_predictive_density(val)
    print(l1["elpd_loo"], l1["se"], l3["elpd_loo"], l3["se"], e1["elpd"], e3["elpd"])
    assert l3["elpd_loo"] - l1["elpd_loo"] > max(l3["se"], l1["se"])
    assert e3["elpd"] > e1["elpd"]
