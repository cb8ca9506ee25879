"""Scoring a Student-t fit with a nu per draw on the MI355X (``nu_draws=`` of pybmc_amd.scoring;
bmc_pointwise_loglik_tv, bmc_psis_loo_tv; TileDrawsTV of bmc_score_tile.h) against the dense numpy
reference of tests/tscore_nu_reference.py.

Bars (tscore_nu_reference.BAR_*), formed by the rule of test_tscore_gpu.py: 100 x the rounding floor
of the float64 reference against np.longdouble on these very cases
(test_tscore_nu_host.py::test_reference_rounding_floor):

    lppd          1e-11 max(1, |ref|), the bar of test_scoring_gpu.py   (floor here 9.9e-16)
    p_waic_i      1e-11 relative (+1e-24), the same                      (floor 6.0e-16)
    mean_ll_i     1e-11 relative (+1e-24), the same                      (floor 2.8e-16)
    elpd_loo_i    9.0e-14 max(1, |ref|)                                  (floor 9.0e-16)
    pareto_k      3.4e-13 absolute, infinite where the reference's is    (floor 3.4e-15)

Measured on one MI355X over the four cases: lppd 1.1e-15, p_waic_i 5.2e-16, mean_ll_i 3.4e-16,
elpd_loo_i 1.1e-15, pareto_k 3.2e-15.
"""
import os

import numpy as np
import pytest

import tscore_nu_reference as TV
import tscore_reference as T

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PW_KEYS = ("lppd", "p_waic", "mean_ll")
LOO_KEYS = ("elpd_loo", "pareto_k", "lppd")


def plw(*a, **kw):
    from pybmc_amd import pointwise_log_likelihood
    return pointwise_log_likelihood(*a, **kw)


def loo_raw(A, y, th, **kw):
    from pybmc_amd import psis_loo
    out = psis_loo(A, y, th, **kw)
    assert np.array_equal(out["p_loo_i"], out["lppd"] - out["elpd_loo_i"], equal_nan=True)
    return {"elpd_loo": out["elpd_loo_i"], "pareto_k": out["pareto_k"], "lppd": out["lppd"]}


@pytest.mark.parametrize("k,n,S", TV.SHAPES)
def test_one_value_for_all_draws_is_the_scalar_call(k, n, S):
    """nu_draws = full(S, 4.0) gives the bits of nu = 4.0, with host arrays and with device tensors."""
    import torch
    from pybmc_amd import waic
    A, y, th = T.shape_case(k, n, S)
    nu = np.full(S, 4.0)
    pw, loo = plw(A, y, th, nu=4.0), loo_raw(A, y, th, nu=4.0)
    thd = torch.as_tensor(th, device=torch.device("cuda", 0))
    for draws in (th, thd):
        got, gloo = plw(A, y, draws, nu_draws=nu), loo_raw(A, y, draws, nu_draws=nu)
        for key in PW_KEYS:
            assert np.array_equal(got[key], pw[key]), key
        for key in LOO_KEYS:
            assert np.array_equal(gloo[key], loo[key]), key
    w = waic(A, y, th, nu_draws=nu)
    assert np.array_equal(w["p_waic_i"], pw["p_waic"]) and np.array_equal(w["mean_ll"], pw["mean_ll"])
    if S >= 25:
        assert np.isfinite(loo["pareto_k"]).all()


@pytest.mark.parametrize("k,n,S", TV.SHAPES)
def test_cycling_nu_against_the_reference(k, n, S):
    A, y, th = T.shape_case(k, n, S)
    nu = TV.cycling_nu(S)
    ref = TV.reference(k, n, S)
    got = (plw(A, y, th, nu_draws=nu), loo_raw(A, y, th, nu_draws=nu))
    d = T.deviations(got, *ref)
    print(f"k={k} n={n} S={S}", " ".join(f"{key} {v:.3e}" for key, v in d.items()))
    assert all(np.isfinite(ref[0][key]).all() for key in PW_KEYS) and np.isfinite(ref[1]["elpd_loo"]).all()
    assert d["lppd"] <= TV.BAR_LPPD and d["p_waic"] <= TV.BAR_REL and d["mean_ll"] <= TV.BAR_REL, d
    assert d["loo_lppd"] <= TV.BAR_LPPD and d["elpd_loo"] <= TV.BAR_ELPD and d["pareto_k"] <= TV.BAR_K, d
    # chains: (C, T) draws of nu pooled like the samples, burn and thin applied to both
    if S == 130:
        pooled = plw(A, y, th.reshape(2, 65, k + 1), nu_draws=nu.reshape(2, 65), burn=5, thin=2)
        keep = np.r_[np.arange(5, 65, 2), 65 + np.arange(5, 65, 2)]
        flat = plw(A, y, np.ascontiguousarray(th[keep]), nu_draws=nu[keep])
        for key in PW_KEYS:
            assert np.array_equal(pooled[key], flat[key]), key


def test_repeatable_and_independent_of_the_order_of_the_draws():
    k, n, S = 4, 65, 130
    A, y, th = T.shape_case(k, n, S)
    nu = TV.cycling_nu(S)
    a, b = loo_raw(A, y, th, nu_draws=nu), loo_raw(A, y, th, nu_draws=nu)
    pa, pb = plw(A, y, th, nu_draws=nu), plw(A, y, th, nu_draws=nu)
    for key in LOO_KEYS:
        assert np.array_equal(a[key], b[key]), key
    for key in PW_KEYS:
        assert np.array_equal(pa[key], pb[key]), key
    perm = np.random.default_rng(5).permutation(S)
    # what psis_loo promises of the order of the draws (test_psis_gpu.py): the values alone decide, so
    # the permuted call meets the same reference at the same bars (sums over the draws are re-ordered)
    c = loo_raw(A, y, np.ascontiguousarray(th[perm]), nu_draws=nu[perm])
    pc = plw(A, y, np.ascontiguousarray(th[perm]), nu_draws=nu[perm])
    d = T.deviations((pc, c), *TV.reference(k, n, S))
    print("permuted", " ".join(f"{key} {v:.3e}" for key, v in d.items()))
    assert d["lppd"] <= TV.BAR_LPPD and d["p_waic"] <= TV.BAR_REL and d["mean_ll"] <= TV.BAR_REL, d
    assert d["loo_lppd"] <= TV.BAR_LPPD and d["elpd_loo"] <= TV.BAR_ELPD and d["pareto_k"] <= TV.BAR_K, d
    assert np.max(np.abs(a["elpd_loo"] - c["elpd_loo"])) <= 2 * TV.BAR_ELPD * np.max(np.abs(a["elpd_loo"]))
    # permuting nu alone is another fit
    d = loo_raw(A, y, th, nu_draws=nu[perm])
    assert not np.array_equal(a["elpd_loo"], d["elpd_loo"])


def test_c_abi_refusals_leave_the_context_usable():
    import torch
    from pybmc_amd import _lib
    ctx = _lib.default_context(0)
    A, y, th = T.shape_case(4, 63, 25)
    idx = (np.arange(25) % 3).astype(np.int32)
    vals = np.array(TV.CYCLE)
    dev = torch.device("cuda", 0)
    Ad, yd, td = (torch.as_tensor(v, device=dev) for v in (A, y, th))
    torch.cuda.synchronize()
    with ctx.lock:
        for call in (ctx.pointwise_loglik_tv, ctx.psis_loo_tv):
            for bad in (0.0, -1.0, float("nan"), float("inf")):
                with pytest.raises(ValueError, match="nu_values must be positive and finite"):
                    call(A, 63, 4, 4, 0, y, th, 25, 5, [1.5, bad, 50.0], idx)
            with pytest.raises(ValueError, match="n_values"):
                call(A, 63, 4, 4, 0, y, th, 25, 5, [], idx)
            for bad in (-1, 3):
                with pytest.raises(ValueError, match="nu_index must index"):
                    call(A, 63, 4, 4, 0, y, th, 25, 5, vals, np.r_[idx[:24], bad].astype(np.int32))
        for call in (ctx.pointwise_loglik_tv_device, ctx.psis_loo_tv_device):
            for bad in (-7, 3, 2 ** 30):          # clamped where it is read, reported afterwards
                bidx = torch.as_tensor(np.r_[idx[:24], bad].astype(np.int32), device=dev)
                torch.cuda.synchronize()
                with pytest.raises(ValueError, match="nu_index must index"):
                    call(Ad.data_ptr(), 63, 4, 4, 0, yd.data_ptr(), td.data_ptr(), 25, 5, vals, bidx.data_ptr())
        good = torch.as_tensor(idx, device=dev)
        torch.cuda.synchronize()
        on_dev = ctx.pointwise_loglik_tv_device(Ad.data_ptr(), 63, 4, 4, 0, yd.data_ptr(), td.data_ptr(), 25,
                                                5, vals, good.data_ptr())
        on_host = ctx.pointwise_loglik_tv(A, 63, 4, 4, 0, y, th, 25, 5, vals, idx)
    ref = TV.reference(4, 63, 25)[0]
    for key in PW_KEYS:
        assert np.array_equal(on_dev[key], on_host[key]), key
    assert T.deviations((on_host, None), ref, None)["lppd"] <= TV.BAR_LPPD


def test_score_of_an_estimated_fit_on_the_standin_dataset():
    from pybmc_amd import BayesianModelCombination, Dataset, compare_elpd, psis_loo
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
    b.train({"sampler": "student_t", "nu": "estimate", "iterations": 3000, "n_chains": 2, "seeds": [7, 8]})
    t = b.score("loo", burn=100)
    nus = b.nu_samples.reshape(2, 3000)
    assert t["likelihood"] == "student_t" and t["nu_estimated"] is True and t["n_draws"] == 5800
    assert t["nu"] == pytest.approx(float(nus[:, 100:].mean()), rel=1e-14)
    direct = psis_loo(b.U_hat, yc, b.samples.reshape(2, 3000, 4), burn=100, nu_draws=nus)
    assert np.array_equal(t["elpd_loo_i"], direct["elpd_loo_i"]) and np.isfinite(t["elpd_loo"])
    tw = b.score("waic")
    assert tw["nu_estimated"] is True and np.isfinite(tw["elpd_waic"])
    held = b.score(X=val_df)
    assert held["n_points"] == len(val_df) and np.isfinite(held["lppd"]).all()
    out = compare_elpd({"gaussian": g, "student_t_nu": t})
    assert sorted(out["names"]) == ["gaussian", "student_t_nu"] and np.isfinite(out["se_diff"]).all()
    with pytest.raises(ValueError, match="supports the Gaussian Gibbs sampler only"):
        b.loo_predict()
