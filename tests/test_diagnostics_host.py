"""Convergence diagnostics without a GPU: the numpy reference estimator on processes with known
answers, argument checks that raise before any device is touched, and the plumbing of
BayesianModelCombination.diagnostics() with the device call stood in by the reference."""
import numpy as np
import pandas as pd
import pytest

import diag_reference as R
from pybmc_amd import chain_diagnostics
from pybmc_amd import bmc as bmc_mod
from pybmc_amd.diagnostics import KEYS, lag_blocks


def test_reference_iid_chains():
    rng = np.random.default_rng(1)
    d = R.diagnostics(rng.standard_normal((4, 4000, 3)))
    Mn = 8 * 2000
    assert np.all(np.abs(d["ess"] / Mn - 1) < 0.10), d["ess"]
    assert np.all(d["r_hat"] < 1.01)
    assert np.allclose(d["mcse_mean"], d["sd"] / np.sqrt(d["ess"]))


def test_reference_ar1_ess():
    rng = np.random.default_rng(2)
    phi = 0.9
    d = R.diagnostics(R.ar1(rng, 4, 20000, 2, phi))
    expect = 8 * 10000 * (1 - phi) / (1 + phi)
    assert np.all(np.abs(d["ess"] / expect - 1) < 0.15), (d["ess"], expect)
    assert np.all(d["max_lag"] > 10)


def test_reference_shifted_chains():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((4, 1000, 2)) + np.array([0.0, 0.0, 1.0, 1.0])[:, None, None]
    assert np.all(R.diagnostics(x)["r_hat"] > 1.1)


def test_reference_degenerate_columns():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((2, 100, 3))
    x[:, :, 1] = 5.0
    x[1, 70, 2] = np.nan
    d = R.diagnostics(x)
    assert np.isfinite(d["r_hat"][0]) and np.isnan(d["r_hat"][1:]).all()
    assert np.isnan(d["ess"][1:]).all() and np.isnan(d["mcse_mean"][1:]).all()


@pytest.mark.parametrize("shape,burn", [((3, 7, 2), 0), ((20, 2), 13), ((2, 10, 1), 3)])
def test_too_few_draws_after_burn(shape, burn):
    with pytest.raises(ValueError, match="n = "):
        chain_diagnostics(np.zeros(shape), burn=burn)


def test_bad_rank_dtype_and_burn():
    with pytest.raises(ValueError, match="dimensions"):
        chain_diagnostics(np.zeros(100))
    with pytest.raises(ValueError, match="dimensions"):
        chain_diagnostics(np.zeros((2, 2, 100, 3)))
    with pytest.raises(ValueError, match="float64"):
        chain_diagnostics(np.zeros((100, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="float64"):
        chain_diagnostics(np.zeros((100, 3), dtype=np.int64))
    with pytest.raises(ValueError, match="burn"):
        chain_diagnostics(np.zeros((100, 3)), burn=-1)


def test_lag_blocks_follow_the_doubling_schedule():
    assert lag_blocks([1, 5, 63], 1000) == 1
    assert lag_blocks([64], 1000) == 2
    assert lag_blocks([191], 1000) == 2
    assert lag_blocks([192], 1000) == 3
    assert lag_blocks([998], 1000) == 5      # 64 + 128 + 256 + 512 > 998: clipped at n


def _trained_bmc(monkeypatch, n_chains, T):
    """A BayesianModelCombination in the state train() leaves (no GPU): pooled chain-major
    samples, n_chains recorded; the device diagnostics replaced by the numpy reference."""
    rng = np.random.default_rng(5)
    df = pd.DataFrame({"m1": rng.normal(size=30), "m2": rng.normal(size=30),
                       "m3": rng.normal(size=30), "truth": rng.normal(size=30)})
    b = bmc_mod.BayesianModelCombination(["m1", "m2", "m3"], {"p": df}, "truth")
    b.orthogonalize("p", df, 2, method="svd")
    chains = rng.standard_normal((n_chains, T, 3)) + np.arange(n_chains)[:, None, None] * 0.01
    b.samples = chains.reshape(-1, 3) if n_chains > 1 else chains[0]
    b.n_chains = n_chains
    calls = []

    def fake(samples, Vt_hat, burn, device):
        calls.append((samples.shape, burn))
        w = samples[..., :-1] @ Vt_hat + 1.0 / Vt_hat.shape[1]
        return R.diagnostics(np.concatenate([samples, w], axis=-1), burn=burn)

    monkeypatch.setattr(bmc_mod, "_series_diagnostics", fake)
    return b, chains, calls


@pytest.mark.parametrize("n_chains", [1, 3])
def test_bmc_diagnostics_frame(monkeypatch, n_chains):
    T = 400
    b, chains, calls = _trained_bmc(monkeypatch, n_chains, T)
    df = b.diagnostics(burn=20)
    assert calls == [((n_chains, T, 3), 20)]          # pooled samples split back by chain
    assert list(df.index) == ["beta_0", "beta_1", "sigma", "m1", "m2", "m3"]
    assert list(df.columns) == list(KEYS)
    w = chains[:, 20:, :2] @ b.Vt_hat + 1.0 / 3
    assert np.allclose(df.loc[["m1", "m2", "m3"], "mean"], w.reshape(-1, 3).mean(0), rtol=1e-12)
    assert np.allclose(df.loc["sigma", "mean"], chains[:, 20:, 2].mean(), rtol=1e-12)
    ref = R.diagnostics(chains, burn=20)
    assert np.allclose(df["r_hat"].to_numpy()[:3], ref["r_hat"], rtol=1e-12)


def test_bmc_diagnostics_needs_train():
    df = pd.DataFrame({"m1": [1.0, 2.0], "m2": [3.0, 4.0], "truth": [5.0, 6.0]})
    b = bmc_mod.BayesianModelCombination(["m1", "m2"], {"p": df}, "truth")
    assert b.n_chains is None
    with pytest.raises(ValueError, match="Must call .*train()"):
        b.diagnostics()
