"""Scoring a Student-t fit on the MI355X (``nu=`` of pybmc_amd.scoring; bmc_pointwise_loglik_t,
bmc_psis_loo_t; TileDrawsT of bmc_score_tile.h) against the dense numpy reference of
tests/tscore_reference.py.

Bars (tscore_reference.BAR_*): 100 x the rounding floor of the float64 reference against
np.longdouble, re-measured on these very cases by test_tscore_host.py::test_reference_rounding_floor:

    lppd          1e-11 max(1, |ref|), the bar of test_scoring_gpu.py   (floor here 1.6e-15)
    p_waic_i      1e-11 relative (+1e-24), the same                      (floor 1.8e-15)
    mean_ll_i     1e-11 relative (+1e-24), the same                      (floor 4.2e-16)
    elpd_loo_i    2.1e-13 max(1, |ref|)                                  (floor 1.7e-15)
    pareto_k      3.4e-12 absolute, infinite where the reference's is    (floor 2.5e-14)

The tiny-argument case keeps what the issue sets (residuals down to 1e-20, sigma about 1), but no
bar above can tell log1p from a naive log(1 + x) there: the density adds c_s = C(nu) - log sigma_s,
about -1, to -(nu + 1)/2 log1p(x), and the naive form's defect is an ABSOLUTE error of 1.1e-16 in
the logarithm, i.e. 3e-16 of |ll|.  What holds log1p_nonneg to its relative accuracy at small
arguments is test_tscore_host.py::test_log1p_nonneg_against_libm, on the text the kernels compile.

Measured on one MI355X over all cases of this file: lppd 1.3e-15, p_waic_i 1.8e-15, mean_ll_i
5.6e-16, elpd_loo_i 2.7e-15, pareto_k 2.3e-14; the planted 200 x 3 problem: elpd_loo +77.5 (t,
nu = 4) against -45.1 (Gaussian), difference 122.6 = 10.1 se_diff, largest pareto_k 0.18 / 0.60."""
import os

import numpy as np
import pytest

import psis_reference as P
import robust_cases as RC
import score_reference as R
import tscore_reference as T
from conftest import load_golden

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def check(got_pw, got_loo, ref, tag):
    """Both results of a case against its reference; prints the figures before it asserts."""
    d = T.deviations((got_pw, got_loo), *ref)
    print(tag, " ".join(f"{k} {v:.3e}" for k, v in d.items()))
    if got_pw is not None:
        assert all(np.isfinite(ref[0][k]).all() for k in ("lppd", "p_waic", "mean_ll")), tag
        assert d["lppd"] <= T.BAR_LPPD and d["p_waic"] <= T.BAR_REL and d["mean_ll"] <= T.BAR_REL, (tag, d)
    if got_loo is not None:
        assert np.isfinite(ref[1]["elpd_loo"]).all(), tag
        assert d["loo_lppd"] <= T.BAR_LPPD and d["elpd_loo"] <= T.BAR_ELPD and d["pareto_k"] <= T.BAR_K, (tag, d)


def loo_raw(A, y, th, **kw):
    from pybmc_amd import psis_loo
    out = psis_loo(A, y, th, **kw)
    assert np.array_equal(out["p_loo_i"], out["lppd"] - out["elpd_loo_i"], equal_nan=True)
    return {"elpd_loo": out["elpd_loo_i"], "pareto_k": out["pareto_k"], "lppd": out["lppd"]}


def plw(*a, **kw):
    from pybmc_amd import pointwise_log_likelihood
    return pointwise_log_likelihood(*a, **kw)


# ---- 1. shapes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu", T.NUS)
def test_shapes_on_both_sides_of_every_rule(nu):
    """k across the 4-column MFMA step and the 16-column slab; points across the 64-wide tile; draws
    with lanes that hold none (2, 24, 25, 63), below and at the M >= 5 rule (24, 25), all of them
    candidates (<= 513: 9 draw tiles in two splits) and, once, the radix select over many splits
    (4097); both layouts, lda and ldt wider than the rows, through the Context methods."""
    from pybmc_amd import _lib
    ctx = _lib.default_context(0)
    for case, (k, n, S) in enumerate(T.SHAPES):
        A, y, th = T.shape_case(k, n, S)
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
            pw = ctx.pointwise_loglik_t(buf, n, k, lda, layout, y, tb, S, k + 1 + pad_t, nu)
            loo = ctx.psis_loo_t(buf, n, k, lda, layout, y, tb, S, k + 1 + pad_t, nu)
        if S < 25:
            assert np.isinf(loo["pareto_k"]).all()
        check(pw, loo, T.reference("shape", (k, n, S), nu),
              f"nu={nu} k={k} n={n} S={S} layout={layout} lda={lda} ldt={k + 1 + pad_t}")


# ---- 2. extreme arguments of log1p ---------------------------------------------------------------------
@pytest.mark.parametrize("nu", T.NUS)
@pytest.mark.parametrize("kind", ["outlier", "tiny"])
def test_extreme_arguments_of_log1p(kind, nu):
    A, y, th = T.case_arrays(kind, None)
    check(plw(A, y, th, nu=nu), loo_raw(A, y, th, nu=nu), T.reference(kind, None, nu), f"{kind} nu={nu}")


# ---- 3. golden chains ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gibbs_ortho629x3", "gibbs_ragged1237x5"])
def test_golden_chains_as_draws(name):
    from pybmc_amd import psis_loo, waic
    g = load_golden(name)
    A, y, th = np.asarray(g["X"], dtype=np.float64), g["y"], g["samples"]
    ref_pw, ref_loo = T.pointwise(A, y, th, 4.0), T.loo_pointwise(A, y, th, 4.0)
    w = waic(np.asfortranarray(A), y, th, nu=4.0)
    for key, v in R.waic_summary(ref_pw).items():
        assert w[key] == pytest.approx(v, rel=1e-9), key
    out = psis_loo(A, y, th, nu=4.0)
    for key, v in P.loo_summary(ref_loo, len(th)).items():
        assert out[key] == pytest.approx(v, rel=1e-9), key
    # and the density is not the Gaussian one
    assert abs(waic(A, y, th)["elpd_waic"] - w["elpd_waic"]) > 1.0


# ---- 4. bits -----------------------------------------------------------------------------------------------
def test_deterministic_host_equals_device_and_views_equal_copies():
    import torch
    from pybmc_amd import _lib
    A, y, th = R.random_case(130, 5, 4097, 21)
    nu = 4.0
    a, b = plw(A, y, th, nu=nu), plw(A, y, th, nu=nu)
    la, lb = loo_raw(A, y, th, nu=nu), loo_raw(A, y, th, nu=nu)
    dev = torch.device("cuda", 0)
    wide = torch.full((4097, 9), float("nan"), dtype=torch.float64, device=dev)
    wide[:, :6] = torch.as_tensor(th, device=dev)
    view = wide[:, :6]
    assert view.stride(0) == 9
    c, lc = plw(A, y, view, nu=nu), loo_raw(A, y, view, nu=nu)
    Ad = torch.as_tensor(np.asfortranarray(A).T.copy(), device=dev)   # column-major on the device
    yd = torch.as_tensor(y, device=dev)
    torch.cuda.synchronize()
    ctx = _lib.default_context(0)
    with ctx.lock:
        d = ctx.pointwise_loglik_t_device(Ad.data_ptr(), 130, 5, 130, _lib.BMC_COL_MAJOR,
                                          yd.data_ptr(), wide.data_ptr(), 4097, 9, nu)
        ld = ctx.psis_loo_t_device(Ad.data_ptr(), 130, 5, 130, _lib.BMC_COL_MAJOR, yd.data_ptr(),
                                   wide.data_ptr(), 4097, 9, nu)
    for key in a:
        assert np.array_equal(a[key], b[key]) and np.array_equal(a[key], c[key]), key
        assert np.array_equal(a[key], d[key]), key
    for key in la:
        assert np.array_equal(la[key], lb[key]) and np.array_equal(la[key], lc[key]), key
        assert np.array_equal(la[key], ld[key]), key
    # a column subset (one strided run of rows) and thinned draws, read in place, against the copy
    big = np.full((4097, 11), np.nan)
    big[:, 2:8] = th
    sub = big[:, 2:8]
    assert not sub.flags.c_contiguous
    for key, v in plw(A, y, sub, nu=nu).items():
        assert np.array_equal(v, a[key]), key
    thin_pw, thin_loo = plw(A, y, th, thin=3, nu=nu), loo_raw(A, y, th, thin=3, nu=nu)
    copy = np.ascontiguousarray(th[::3])
    for key, v in plw(A, y, copy, nu=nu).items():
        assert np.array_equal(v, thin_pw[key]), key
    for key, v in loo_raw(A, y, copy, nu=nu).items():
        assert np.array_equal(v, thin_loo[key]), key


# ---- 5. non-finite values ------------------------------------------------------------------------------------
def test_non_finite_values_are_values():
    A, y, th = R.random_case(130, 5, 513, 9)
    nu = 4.0
    ref_pw, ref_loo = T.pointwise(A, y, th, nu), T.loo_pointwise(A, y, th, nu)
    pw_keys, loo_keys = ("lppd", "p_waic", "mean_ll"), ("elpd_loo", "pareto_k", "lppd")

    def one_point(A2, y2, i, bad):
        ok = np.arange(130) != i
        got, loo = plw(A2, y2, th, nu=nu), loo_raw(A2, y2, th, nu=nu)
        for key in pw_keys:
            assert np.isnan(got[key][i]) if np.isnan(bad) else not np.isfinite(got[key][i]), (key, bad)
            np.testing.assert_allclose(got[key][ok], ref_pw[key][ok], rtol=1e-10)
        for key in loo_keys:
            assert np.isnan(loo[key][i]) if np.isnan(bad) else not np.isfinite(loo[key][i]), (key, bad)
            np.testing.assert_allclose(loo[key][ok], ref_loo[key][ok], rtol=1e-10)

    for bad in (np.nan, np.inf, -np.inf):
        A2 = A.copy()
        A2[17, 2] = bad
        one_point(A2, y, 17, bad)
        y2 = y.copy()
        y2[70] = bad
        one_point(A, y2, 70, bad)
    for row, col, val in ((333, 1, np.nan), (512, 5, 0.0), (0, 5, -0.3), (64, 5, np.nan)):
        t2 = th.copy()
        t2[row, col] = val
        got, loo = plw(A, y, t2, nu=nu), loo_raw(A, y, t2, nu=nu)
        for key in pw_keys:
            assert np.isnan(got[key]).all(), (key, row, col, val)
        for key in loo_keys:
            assert np.isnan(loo[key]).all(), (key, row, col, val)


# ---- 6. ABI ----------------------------------------------------------------------------------------------------
def test_c_abi_refuses_a_bad_nu_and_stays_usable():
    from pybmc_amd import _lib
    ctx = _lib.default_context(0)
    A, y, th = T.shape_case(4, 63, 25)
    ref = T.reference("shape", (4, 63, 25), 4.0)
    for call in (ctx.pointwise_loglik_t, ctx.psis_loo_t):
        for nu in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="nu must be positive and finite"):
                call(A, 63, 4, 4, 0, y, th, 25, 5, nu)
        with pytest.raises(ValueError, match="ldt"):          # the other checks are the siblings'
            call(A, 63, 4, 4, 0, y, th, 25, 4, 4.0)
    check(ctx.pointwise_loglik_t(A, 63, 4, 4, 0, y, th, 25, 5, 4.0),
          ctx.psis_loo_t(A, 63, 4, 4, 0, y, th, 25, 5, 4.0), ref, "after the refusals")
    # the Gaussian call next to it is the Gaussian call still
    g = ctx.pointwise_loglik(A, 63, 4, 4, 0, y, th, 25, 5)
    want = R.pointwise(A, y, th)
    np.testing.assert_allclose(g["lppd"], want["lppd"], rtol=1e-11)


# ---- 7. end to end -------------------------------------------------------------------------------------------------
def test_planted_outliers_prefer_the_t_fit():
    """The question the feature is for: elpd_loo of the Student-t fit next to the Gaussian fit's on
    the planted 200 x 3 problem.  The float64 references on host variates give a difference of
    10.1 se_diff; the device chains differ from those by their variates only."""
    from pybmc_amd import compare_elpd, gibbs_sampler, gibbs_sampler_robust, psis_loo
    y, X, prior, _, idx = RC.planted("200x3")
    seeds = [41, 42, 43, 44]
    t_draws = gibbs_sampler_robust(y, X, RC.PLANTED_KEEP, prior, 4.0, burn=RC.PLANTED_BURN, n_chains=4,
                                   seeds=seeds)
    g_draws = gibbs_sampler(y, X, RC.PLANTED_BURN + RC.PLANTED_KEEP, prior, n_chains=4, seeds=seeds)
    gauss = psis_loo(X, y, g_draws, burn=RC.PLANTED_BURN, nu=None)
    t = psis_loo(X, y, t_draws, nu=4.0)
    cmp_ = compare_elpd({"gaussian": gauss, "student_t": t})
    print(cmp_, "max k:", t["pareto_k"].max(), gauss["pareto_k"].max(), int(np.argmax(gauss["pareto_k"])))
    assert cmp_["names"] == ["student_t", "gaussian"]
    assert cmp_["elpd_diff"][1] > 4.0 * cmp_["se_diff"][1]
    assert t["n_high_k"] == 0 and np.all(t["pareto_k"] <= 0.7)
    assert int(np.argmax(gauss["pareto_k"])) in set(int(i) for i in idx)


def test_score_on_the_standin_dataset():
    from pybmc_amd import BayesianModelCombination, Dataset, compare_elpd, psis_loo, waic
    models = ["FRDM", "HFB24", "UNEDF1", "SKM"]
    ds = Dataset(os.path.join(GOLDEN, "dataset_standin.csv"))
    data = ds.load_data(models + ["truth"], keys=["BE"], domain_keys=["N", "Z"])
    train_df, val_df, _ = ds.split_data(data, "BE", splitting_algorithm="random", train_size=0.6,
                                        val_size=0.2, test_size=0.2)
    b = BayesianModelCombination(models, data, truth_column_name="truth")
    b.orthogonalize("BE", train_df, components_kept=3, method="svd")
    yc = np.asarray(b.centered_experiment_train, dtype=np.float64)

    b.train({"iterations": 3000, "burn": 500, "n_chains": 2, "seeds": [7, 8]})
    g = b.score()
    assert g["likelihood"] == "gaussian" and g["nu"] is None
    assert np.array_equal(g["elpd_loo_i"], b.loo()["elpd_loo_i"])

    b.train({"sampler": "student_t", "nu": 4, "iterations": 3000, "n_chains": 2, "seeds": [7, 8]})
    t = b.score("loo", burn=100)
    assert t["likelihood"] == "student_t" and t["nu"] == 4.0 and t["n_draws"] == 5800
    chains = b.samples.reshape(2, 3000, 4)
    direct = psis_loo(b.U_hat, yc, chains, burn=100, nu=4.0)
    assert np.array_equal(t["elpd_loo_i"], direct["elpd_loo_i"])
    assert np.array_equal(t["pareto_k"], direct["pareto_k"])
    tw = b.score("waic")
    assert tw["likelihood"] == "student_t" and np.array_equal(
        tw["elpd_waic_i"], waic(b.U_hat, yc, chains, nu=4.0)["elpd_waic_i"])
    held = b.score(X=val_df)
    assert held["likelihood"] == "student_t" and held["n_points"] == len(val_df)
    assert np.isfinite(held["lppd"]).all() and held["elpd"] == pytest.approx(float(np.sum(held["lppd"])))
    out = compare_elpd({"gaussian": g, "student_t": t})
    assert sorted(out["names"]) == ["gaussian", "student_t"] and np.isfinite(out["se_diff"]).all()
    with pytest.raises(ValueError, match="supports the Gaussian Gibbs sampler only"):
        b.waic()


# ---- 8. a nu per draw: the index out of range ------------------------------------------------------------------
def test_tv_refuses_an_index_out_of_range_and_rezeroes_its_flag():
    """n = 65, S = 66, k = 3, two nu values: one full and one partly filled tile on both axes.  A host
    index holding -1 or V is refused before any launch; the same index on the device is clamped in
    the kernel and reported after it; and the valid call that follows on the same context returns
    the bits of a fresh context, so the flag word is zeroed by every call."""
    import torch
    from pybmc_amd import _lib
    n, S, k = 65, 66, 3
    A, y, th = T.shape_case(k, n, S)
    vals = np.array([3.0, 7.5])
    good = (np.arange(S) % 2).astype(np.int32)
    dev = torch.device("cuda", 0)
    Ad, yd, thd = (torch.as_tensor(v, device=dev) for v in (A, y, th))
    good_d = torch.as_tensor(good, device=dev)
    torch.cuda.synchronize()
    ctx, fresh = _lib.Context(0), _lib.Context(0)
    host = lambda c, name, idx: getattr(c, name)(A, n, k, k, 0, y, th, S, k + 1, vals, idx)
    device = lambda c, name, idx_d: getattr(c, name + "_device")(
        Ad.data_ptr(), n, k, k, 0, yd.data_ptr(), thd.data_ptr(), S, k + 1, vals, idx_d.data_ptr())
    for name in ("pointwise_loglik_tv", "psis_loo_tv"):
        want = host(fresh, name, good)
        want_d = device(fresh, name, good_d)
        for key in want:
            assert np.isfinite(want[key]).all() and np.array_equal(want[key], want_d[key]), (name, key)
        for at, bad_value in ((0, -1), (S - 1, len(vals)), (64, -1), (17, len(vals))):
            bad = good.copy()
            bad[at] = bad_value
            with pytest.raises(ValueError, match="nu_index must index nu_values"):
                host(ctx, name, bad)
            for key, v in host(ctx, name, good).items():
                assert np.array_equal(v, want[key]), (name, key, at, bad_value, "host")
            bad_d = torch.as_tensor(bad, device=dev)
            torch.cuda.synchronize()
            with pytest.raises(ValueError, match=r"nu_index must index nu_values \(the results are not valid\)"):
                device(ctx, name, bad_d)
            for key, v in device(ctx, name, good_d).items():
                assert np.array_equal(v, want[key]), (name, key, at, bad_value, "device")
