"""Convergence diagnostics on the GPU (-m gpu): kernels_diag.hip through the C ABI and the
Python API against the numpy FFT reference (tests/diag_reference.py), NaN rules, bitwise
determinism, the host and device entries, and samples straight from the samplers."""
import os

import numpy as np
import pytest

import diag_reference as R
from conftest import GOLDEN
from pybmc_amd import chain_diagnostics

pytestmark = pytest.mark.gpu


def check_against_reference(x, burn=0, got=None):
    got = chain_diagnostics(x, burn=burn) if got is None else got
    ref = R.diagnostics(np.asarray(x), burn=burn)
    ok = np.isfinite(ref["mean"]) & np.isfinite(ref["sd"])
    assert not np.isfinite(got["mean"][~ok] + got["sd"][~ok]).any()
    scale = np.maximum(np.abs(ref["mean"]), ref["sd"])[ok]    # a mean near 0: relative to sd
    assert np.all(np.abs(got["mean"][ok] - ref["mean"][ok]) <= 1e-12 * scale), (got["mean"], ref["mean"])
    np.testing.assert_allclose(got["sd"][ok], ref["sd"][ok], rtol=1e-12, atol=0, err_msg="sd")
    for key, rtol in (("r_hat", 1e-12), ("ess", 1e-9), ("mcse_mean", 1e-9)):
        np.testing.assert_allclose(got[key], ref[key], rtol=rtol, atol=0, equal_nan=True,
                                   err_msg=key)
    np.testing.assert_array_equal(got["max_lag"], ref["max_lag"])
    return got, ref


CASES = {
    "iid": lambda rng: rng.standard_normal((4, 3000, 5)),
    "ar1_0.5": lambda rng: R.ar1(rng, 4, 3000, 3, 0.5),
    "ar1_0.99": lambda rng: R.ar1(rng, 4, 6000, 3, 0.99),
    "ar1_0.999": lambda rng: R.ar1(rng, 2, 20000, 2, 0.999),
    "shifted": lambda rng: rng.standard_normal((4, 1000, 3)) + np.arange(4.0)[:, None, None],
    "large_mean": lambda rng: R.ar1(rng, 4, 2000, 2, 0.3, loc=1e4, scale=1e-2),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_matches_reference(name):
    rng = np.random.default_rng(100 + sorted(CASES).index(name))
    got, ref = check_against_reference(CASES[name](rng))
    if name == "shifted":
        assert np.all(got["r_hat"] > 1.1)
    if name == "ar1_0.999":
        assert got["max_lag"].max() >= 192     # past the first two lag blocks


def test_odd_kept_draws_with_burn():
    rng = np.random.default_rng(11)
    x = R.ar1(rng, 3, 1001, 4, 0.7)
    check_against_reference(x, burn=100)       # T' = 901: the middle draw counts for mean / sd
    check_against_reference(x, burn=0)


# (256, 40, 300): 5 half-chains per autocovariance workgroup, the last group clipped by 3;
# (32, 1400, 100): two 128-row tiles per row split (the classes: tests/test_diag_plan.py)
@pytest.mark.parametrize("C,T,P", [(1, 500, 1), (64, 200, 33), (2, 300, 257), (256, 40, 300),
                                   (32, 1400, 100)])
def test_chain_and_column_counts(C, T, P):
    rng = np.random.default_rng(C * 1000 + P)
    check_against_reference(R.ar1(rng, C, T, P, 0.6), burn=10)


def test_column_subset_ld_greater_than_n_cols():
    import torch
    rng = np.random.default_rng(12)
    full = R.ar1(rng, 3, 800, 9, 0.8)
    sub = full[:, :, 2:7]                       # a view: row stride 9, 5 columns
    check_against_reference(sub)
    t = torch.as_tensor(full, device="cuda:0")[:, :, 2:7]
    assert t.stride() == (800 * 9, 9, 1)
    check_against_reference(sub, got=chain_diagnostics(t))


def test_degenerate_columns_give_nan():
    rng = np.random.default_rng(13)
    x = rng.standard_normal((2, 300, 4))
    x[:, :, 1] = 3.0
    x[0, 10, 2] = np.nan
    x[1, 200, 3] = np.inf
    got, ref = check_against_reference(x)
    assert np.isfinite(got["r_hat"][0]) and np.isfinite(got["ess"][0])
    for key in ("r_hat", "ess", "mcse_mean"):
        assert np.isnan(got[key][1:]).all(), key


def test_bitwise_deterministic_and_host_equals_device():
    import torch
    rng = np.random.default_rng(14)
    x = R.ar1(rng, 8, 4000, 17, 0.95)
    a = chain_diagnostics(x, burn=3)
    b = chain_diagnostics(x, burn=3)
    c = chain_diagnostics(torch.as_tensor(x, device="cuda:0"), burn=3)
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=True), key
        assert np.array_equal(a[key], c[key], equal_nan=True), key


def test_bad_arguments_raise():
    import torch
    with pytest.raises(ValueError, match="n = "):
        chain_diagnostics(torch.zeros((2, 9, 3), dtype=torch.float64, device="cuda:0"), burn=2)
    with pytest.raises(ValueError, match="float64"):
        chain_diagnostics(torch.zeros((2, 90, 3), dtype=torch.float32, device="cuda:0"))
    from pybmc_amd import _lib
    ctx = _lib.default_context(0)
    x = np.zeros((2, 100, 3))
    with pytest.raises(ValueError, match="ld must be >= n_cols"):
        ctx.chain_diagnostics(x, 2, 100, 3, 2)
    with pytest.raises(ValueError, match=">= 4 draws"):
        ctx.chain_diagnostics(x, 2, 100, 3, 3, burn=93)
    with pytest.raises(ValueError, match="n_chains"):
        ctx.chain_diagnostics(x, 0, 100, 3, 3)


def test_run_chains_output_on_the_device():
    from gpu_common import gpu_ctx
    from pybmc_amd.chains import run_chains
    from pybmc_amd.synthetic import synth_problem
    ctx = gpu_ctx()
    p = synth_problem(3000, 6, 5, seed=3)
    ctx.set_problem(p["y"], p["X"])
    ctx.set_prior(*p["prior"])
    pooled, _ = run_chains(ctx, 8, 4000, base_seed=5)
    got = chain_diagnostics(pooled, burn=0)
    assert np.all(got["r_hat"] < 1.01), got["r_hat"]
    check_against_reference(pooled.cpu().numpy(), got=got)


def _standin_bmc():
    from pybmc_amd import BayesianModelCombination, Dataset
    models = ["FRDM", "HFB24", "UNEDF1", "SKM"]
    ds = Dataset(os.path.join(GOLDEN, "dataset_standin.csv"))
    data = ds.load_data(models + ["truth"], keys=["BE"], domain_keys=["N", "Z"])
    train_df, _, _ = ds.split_data(data, "BE", splitting_algorithm="random", train_size=0.6,
                                   val_size=0.2, test_size=0.2)
    b = BayesianModelCombination(models, data, truth_column_name="truth")
    b.orthogonalize("BE", train_df, components_kept=3, method="svd")
    return b, models


def test_bmc_diagnostics_on_the_standin_dataset():
    from pybmc_amd.chains import posterior_summary
    b, models = _standin_bmc()
    b.train({"iterations": 3000, "burn": 0, "n_chains": 4, "seeds": [1, 2, 3, 4]})
    assert b.n_chains == 4
    df = b.diagnostics()
    assert list(df.index) == ["beta_0", "beta_1", "beta_2", "sigma"] + models
    assert list(df.columns) == ["mean", "sd", "mcse_mean", "ess", "r_hat", "max_lag"]
    w = posterior_summary(b.samples, b.Vt_hat)["weights_mean"]
    np.testing.assert_allclose(df.loc[models, "mean"].to_numpy(), w, rtol=1e-12)
    assert np.all(df["r_hat"] < 1.05) and np.all(df["ess"] > 100)
    # the same numbers as the reference estimator on the host-formed series
    s = b.samples.reshape(4, -1, 4)
    series = np.concatenate([s, s[..., :3] @ b.Vt_hat + 1.0 / len(models)], axis=-1)
    ref = R.diagnostics(series)
    np.testing.assert_allclose(df["r_hat"].to_numpy(), ref["r_hat"], rtol=1e-10)
    np.testing.assert_allclose(df["ess"].to_numpy(), ref["ess"], rtol=1e-8)


def test_simplex_chain_mixes_slower_than_gibbs():
    b, _ = _standin_bmc()
    T = 6000
    b.train({"iterations": T, "sampler": "simplex", "burn": 1000, "stepsize": 0.001})
    assert b.n_chains == 1
    simplex = b.diagnostics()
    b.train({"iterations": T, "burn": 0, "n_chains": 1, "seeds": [7]})
    gibbs = b.diagnostics()
    rows = ["beta_0", "beta_1", "beta_2"]
    assert np.all(simplex.loc[rows, "ess"] / T < 0.2 * gibbs.loc[rows, "ess"] / T), (simplex, gibbs)
