"""The leave-one-out predictive moments on the MI355X (kernels_loo.hip's PREDICT passes,
pybmc_amd.scoring.psis_loo_predict) against the dense numpy reference of
tests/loo_predict_reference.py: every point, every output.

elpd_loo_i, pareto_k and lppd are held to the bars of test_psis_gpu.py (its check()).  The bars of
the new outputs are 100 x the rounding floor of the float64 reference against np.longdouble,
measured on these very cases by test_loo_predict_host.py (the margin test_psis_gpu.py uses, for
the same reasons: the device's exp / log / erfc are not correctly rounded, the MFMA and the
reductions sum in another order); the floors are loo_predict_reference.FLOORS:

    loo_mean 1.1e-15 absolute   loo_sd 3.0e-15 absolute   loo_pit 4.2e-16 absolute   ess 5.7e-15 relative
    k > 1:   1.5e-15            6.2e-14           2.3e-16            2.1e-14

Measured on the MI355X over all cases of this file: loo_mean 1.1e-15 (k > 1: 1.3e-15), loo_sd
3.1e-15 (1.9e-14), loo_pit 7.8e-16 (4.4e-16), ess 1.1e-14 (2.3e-14); the mirror case: loo_mean[0]
9.8e-19, loo_pit[0] - 1/2 -5.6e-17.

Points whose reference pareto_k exceeds 1 (the 40-sigma outliers: every weight but a handful is
negligible, and loo_sd is the difference of two sums 1600 times its size) have floors of their
own, FLOORS_BIG, measured the same way.  No point is left out."""
import numpy as np
import pytest

import loo_predict_reference as L
import psis_reference as P
import score_reference as R
from conftest import load_golden
from test_psis_gpu import check as check_psis

pytestmark = pytest.mark.gpu

TOL = {key: 100 * v for key, v in L.FLOORS.items()}
TOL_BIG = {key: 100 * v for key, v in L.FLOORS_BIG.items()}


def distances(got, ref):
    """{key: [n] distance of the device to the reference}, in the units of the floors."""
    out = {}
    for key in L.NEW_KEYS:
        r = np.asarray(ref[key], dtype=np.float64)
        d = np.abs(np.asarray(got[key], dtype=np.float64) - r)
        out[key] = d / r if key == "ess" else d
    return out


def check(got, ref, tag=""):
    """Every point of the case against the reference; prints the figures before it asserts."""
    check_psis(got, ref, tag)
    big = np.asarray(ref["pareto_k"], dtype=np.float64) > 1
    d = distances(got, ref)
    print(f"{tag}: " + "  ".join(
        f"{key} {d[key][~big].max() if (~big).any() else 0:.3e} (k > 1: "
        f"{d[key][big].max() if big.any() else 0:.3e})" for key in L.NEW_KEYS))
    for key in L.NEW_KEYS:
        assert np.isfinite(got[key]).all(), (tag, key)
        assert np.all(d[key][~big] <= TOL[key]), (tag, key)
        assert np.all(d[key][big] <= TOL_BIG[key]), (tag, key)
    assert np.all(got["ess"] >= 1 - 1e-12) and np.all(got["loo_sd"] > 0), tag
    assert np.all((got["loo_pit"] >= 0) & (got["loo_pit"] <= 1)), tag


def raw(A, y, th, **kw):
    """The pointwise outputs under the reference's names, and the whole dict."""
    from pybmc_amd import psis_loo_predict
    out = psis_loo_predict(A, y, th, **kw)
    got = {"elpd_loo": out["elpd_loo_i"], "pareto_k": out["pareto_k"], "lppd": out["lppd"]}
    got.update({key: out[key] for key in L.NEW_KEYS})
    return got, out


def check_summary(out, y, ref, S):
    for key, v in P.loo_summary(ref, S).items():
        assert out[key] == pytest.approx(v, rel=1e-9), key
    s = L.summary(y, ref)
    assert out["loo_rmse"] == pytest.approx(s["loo_rmse"], rel=1e-9)
    assert out["min_ess"] == pytest.approx(s["min_ess"], rel=1e-9)
    assert len(out["pit_coverage"]) == 21


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_synthetic_cases_with_a_far_outlier(name):
    A, y, th = R.synth_case(name)
    ref = L.pointwise(A, y, th)
    got, out = raw(A, y, th)
    check(got, ref, name)
    check_summary(out, y, ref, len(th))
    # the outlier's leave-one-out prediction is the fit of the other points: 40 sigma away
    noise = R.CASES[name][4]
    assert abs(y[0] - out["loo_mean"][0]) > 30 * noise and out["loo_pit"][0] > 1 - 1e-12


@pytest.mark.parametrize("name", P.GOLDEN)
def test_golden_chains_as_draws(name):
    g = load_golden(name)
    A, y, th = np.asarray(g["X"], dtype=np.float64), g["y"], g["samples"]
    ref = L.pointwise(A, y, th)
    got, out = raw(np.asfortranarray(A), y, th)
    check(got, ref, name)
    check_summary(out, y, ref, len(th))


@pytest.mark.parametrize("k", (3, 33))
def test_shapes_on_both_sides_of_every_rule(k):
    """Points across the 64-wide tile; draws below and at the M >= 5 rule (24, 25), lanes without
    a draw, several splits (4097: above the candidate cap, so the select and the bucket pass
    run); both layouts, lda and ldt wider than the rows."""
    from pybmc_amd import _lib
    ctx = _lib.default_context(0)
    for case, n, S, (A, y, th) in P.shape_cases(k):
        ref = L.pointwise(A, y, th)
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
            got = ctx.psis_loo_predict(buf, n, k, lda, layout, y, tb, S, k + 1 + pad_t)
        if S < 25:
            assert np.isinf(got["pareto_k"]).all()
        check(got, ref, f"k={k} n={n} S={S} layout={layout} lda={lda} ldt={k + 1 + pad_t}")


def test_mirror_draws_tie_with_opposite_residuals():
    """Every ll[0, s] occurs twice with opposite r: shared weights give loo_mean[0] = 0 and
    loo_pit[0] = 1/2 whatever slot or rank each copy landed in; weights handed out by index do not
    (the reference's "index" variant is 6.9e-7 and 8.2e-7 off, test_loo_predict_host.py)."""
    A, y, th = L.mirror_case()
    ref = L.pointwise(A, y, th)
    got, _ = raw(A, y, th)
    check(got, ref, "mirror")
    print(got["loo_mean"][0], got["loo_pit"][0] - 0.5)
    assert abs(got["loo_mean"][0]) <= TOL["loo_mean"]
    assert abs(got["loo_pit"][0] - 0.5) <= TOL["loo_pit"]
    got_p, _ = raw(A, y, th[np.random.default_rng(5).permutation(len(th))])
    check(got_p, ref, "mirror, permuted")


def test_a_run_of_ties_across_the_cutoff():
    """The S / 2 ties of test_psis_gpu.py (4500 ties against a cap of 1024: the bucket is one
    repeated value and its payload comes from the bucket pass); the cutoff falls inside the run
    for at least 20 points.  The same draws permuted: the values alone decide."""
    A, y, th = R.random_case(200, 5, 9000, 77)
    rng = np.random.default_rng(3)
    rep = th[0].copy()
    rep[:5] += 0.5
    t2 = th.copy()
    t2[rng.permutation(9000)[:4500]] = rep
    ref = L.pointwise(A, y, t2)
    got, _ = raw(A, y, t2)
    check(got, ref, "S/2 ties")
    got_p, _ = raw(A, y, t2[rng.permutation(9000)])
    check(got_p, ref, "S/2 ties, permuted")
    M = P.tail_length(9000)
    ll = R.loglik(A, y, t2)
    inside = [(np.sort(row)[M] == np.sort(row)[M - 1]) for row in ll]
    assert sum(inside) >= 20


def test_values_within_a_few_ulp_and_a_wide_span():
    A, y, th = R.synth_case("c1")
    A = A.copy()
    A[5] = 0.0
    th = th.copy()[:9000]
    th[:, -1] = 0.5 * (1 + np.arange(9000) % 7 * 2.0 ** -51)
    ref = L.pointwise(A, y, th)
    assert ref["lppd"][0] < -600
    ll5 = R.loglik(A[5:6], y[5:6], th)[0]
    assert 1 < len(np.unique(ll5)) <= 8 and np.ptp(ll5) < 1e-14
    got, _ = raw(A, y, th)
    check(got, ref, "few ulp + wide span")
    assert got["loo_mean"][5] == 0.0          # a_5 = 0: every draw predicts 0


def test_pooling_burn_thin_and_device_tensors():
    import torch
    A, y, th = R.random_case(130, 6, 4 * 3000, 33)
    chains = th.reshape(4, 3000, 7)
    for burn, thin in ((0, 1), (37, 3)):
        ref = L.pointwise(A, y, R.pool(chains, burn, thin))
        got, out = raw(A, y, chains, burn=burn, thin=thin)
        check(got, ref, f"numpy burn={burn} thin={thin}")
        assert out["n_draws"] == len(R.pool(chains, burn, thin))
        got_t, _ = raw(A, y, torch.as_tensor(chains, device="cuda:0"), burn=burn, thin=thin)
        for key in got:
            assert np.array_equal(got[key], got_t[key]), key
    ref = L.pointwise(A, y, chains[2, 50::4])
    check(raw(A, y, torch.as_tensor(chains[2], device="cuda:0"), burn=50, thin=4)[0], ref, "one chain, torch")


def test_two_calls_return_the_same_bits_and_psis_loo_keeps_its_own():
    import torch
    from pybmc_amd import psis_loo
    A, y, th = R.random_case(500, 12, 9000, 21)
    a, _ = raw(A, y, th)
    b, _ = raw(A, y, th)
    c, _ = raw(A, y, torch.as_tensor(th, device="cuda:0"))
    for key in a:
        assert np.array_equal(a[key], b[key]), key
        assert np.array_equal(a[key], c[key]), key
    plain = psis_loo(A, y, th)
    for key, pk in (("elpd_loo", "elpd_loo_i"), ("pareto_k", "pareto_k"), ("lppd", "lppd")):
        assert np.array_equal(a[key], plain[pk]), key     # the same weights, the same bits
    check(a, L.pointwise(A, y, th), "determinism case")


def test_non_finite_values_are_values():
    A, y, th = R.random_case(200, 5, 7000, 9)
    ref = L.pointwise(A, y, th)
    keys = [k for k in L.KEYS]
    A2 = A.copy()
    A2[17, 2] = np.nan
    got, _ = raw(A2, y, th)
    ok = np.arange(200) != 17
    for key in keys:
        assert np.isnan(got[key][17]), key
        np.testing.assert_allclose(got[key][ok], np.asarray(ref[key], dtype=np.float64)[ok], rtol=1e-9)
    y2 = y.copy()
    y2[130] = np.inf
    got, _ = raw(A, y2, th)
    ok = np.arange(200) != 130
    for key in keys:
        assert np.isnan(got[key][130]), key
        np.testing.assert_allclose(got[key][ok], np.asarray(ref[key], dtype=np.float64)[ok], rtol=1e-9)
    for row, col, val in ((333, 1, np.nan), (6999, 5, 0.0)):
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
            ctx.psis_loo_predict(*args)
    # past the draw limit of the pair sort: refused by the plan, with the limit in the message;
    # nothing is read (the arrays are far too short for the draw count named)
    with pytest.raises(ValueError, match="1863225"):
        ctx.psis_loo_predict_device(1, 10, 3, 3, 0, 1, 1, 1863226, 4)


# ---- the BayesianModelCombination surface ---------------------------------------------------------
def _fit(kept, chains):
    from pybmc_amd import BayesianModelCombination
    train, models = R.three_component_frame(400, seed=1)
    b = BayesianModelCombination(models, {"p": train}, truth_column_name="truth")
    with pytest.raises(ValueError, match="orthogonalize"):
        b.loo_predict()
    b.orthogonalize("p", train, components_kept=kept, method="svd")
    b.train({"iterations": 3000, "burn": 500, "n_chains": chains, "seeds": list(range(1, chains + 1))})
    return b, train


@pytest.mark.parametrize("chains", [1, 4])
def test_bmc_loo_predict(chains):
    from pybmc_amd import psis_loo_predict
    b, train = _fit(3, chains)
    a = b.loo_predict()
    s = np.asarray(b.samples).reshape(chains, -1, 4)
    yc = np.asarray(b.centered_experiment_train, dtype=np.float64)
    w = psis_loo_predict(b.U_hat, yc, s)
    for key, v in w.items():
        assert np.array_equal(a[key], v), key
    assert np.array_equal(a["predicted"], a["loo_mean"] + b._predictions_mean_train)
    # (the sum is rounded once: eps x the truth's size, 10 to 20 here)
    np.testing.assert_allclose(a["predicted"] - b._predictions_mean_train, a["loo_mean"], rtol=0, atol=1e-14)
    np.testing.assert_allclose(a["truth"], train["truth"].to_numpy(), rtol=0, atol=1e-13)
    np.testing.assert_allclose(a["residual"], yc - a["loo_mean"], rtol=0, atol=0)
    ref = L.pointwise(b.U_hat, yc, s.reshape(-1, 4))
    got = {"elpd_loo": a["elpd_loo_i"], "pareto_k": a["pareto_k"], "lppd": a["lppd"]}
    got.update({key: a[key] for key in L.NEW_KEYS})
    check(got, ref, "bmc.loo_predict")
    # out of sample is no better than in sample
    post = np.asarray(b.U_hat) @ s.reshape(-1, 4)[:, :3].mean(axis=0)
    assert a["loo_rmse"] >= np.sqrt(np.mean((yc - post) ** 2))
    assert a["loo_rmse"] == pytest.approx(np.sqrt(np.mean(a["residual"] ** 2)), rel=1e-12)
    cov = a["pit_coverage"]
    assert len(cov) == 21 and cov[0] == 0 and cov[-1] == 100 and np.all(np.diff(cov) >= 0)
    ab = b.loo_predict(burn=200)
    refb = L.pointwise(b.U_hat, yc, R.pool(s, 200))
    gotb = {"elpd_loo": ab["elpd_loo_i"], "pareto_k": ab["pareto_k"], "lppd": ab["lppd"]}
    gotb.update({key: ab[key] for key in L.NEW_KEYS})
    check(gotb, refb, "bmc.loo_predict(burn)")
