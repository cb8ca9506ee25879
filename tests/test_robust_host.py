"""CPU checks of the Student-t (outlier-robust) sampler: the numpy reference of the sweep
(tests/robust_reference.py) against the statistics it exists for, the accept / reject margins of
the STREAM_ROBUST variates the device-RNG GPU test relies on, and the surface (export, argument
errors before any device work, declaration and binding of bmc_robust_run)."""
import os
import re

import numpy as np
import pytest

import pybmc_amd
from pybmc_amd import _lib

import rng_reference as R
import robust_cases as RC
import robust_reference as RR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "pybmc_amd.h")


@pytest.mark.parametrize("name", sorted(RC.PLANTED))
def test_reference_finds_the_planted_rows(name):
    """nu = 4, burn 200, 1800 kept sweeps.  Measured with these seeds: planted rows' mean lambda at
    most 0.062 (200x3) and 0.120 (333x8), clean median 1.12 and 1.13, sigma ratio 0.34 and 0.34."""
    y, X, prior, _, idx = RC.planted(name)
    n, k = X.shape
    xi, g, gl = RR.host_variates(n, k, RC.PLANTED_BURN + RC.PLANTED_KEEP, 4.0, prior[2], seed=77)
    out, lam = RR.chain(y, X, RC.PLANTED_KEEP, prior, 4.0, xi, g, gl, burn=RC.PLANTED_BURN)
    gauss, _ = RR.chain(y, X, RC.PLANTED_KEEP, prior, 4.0, xi, g, gl, burn=RC.PLANTED_BURN, freeze=True)
    clean = np.setdiff1d(np.arange(n), idx)
    assert len(idx) == int(RC.PLANTED[name][2] * n)
    assert lam[idx].max() < 0.2
    assert np.median(lam[clean]) > 0.9
    assert out[:, k].mean() < 0.5 * gauss[:, k].mean()


def test_frozen_weights_are_the_gaussian_conditionals():
    """With lambda frozen at 1 the sweep is the Gaussian sampler's: beta | sigma2 has the moments of
    the reference's draw (mean Q^-1 rhs, and xi = 0 gives exactly that mean)."""
    y, X, prior = RC.problem(65, 1)
    T = 5
    xi, g, gl = np.zeros((T, 1)), np.full(T, (prior[2] + 65) / 2), np.ones((T, 65))
    out, lam = RR.chain(y, X, T, prior, 4.0, xi, g, gl, freeze=True)
    assert np.array_equal(lam, np.ones(65))
    P = np.linalg.inv(prior[1])
    s2 = max(np.mean((y - X @ np.linalg.solve(X.T @ X, X.T @ y)) ** 2), 1e-6)
    mean = np.linalg.solve(X.T @ X / s2 + P + 1e-6 * np.eye(1), P @ prior[0] + X.T @ y / s2)
    assert abs(out[0, 0] - mean[0]) <= 1e-13 * abs(mean[0])


def test_robust_stream_margins_of_the_device_seeds():
    """No STREAM_ROBUST attempt of the device-RNG GPU test (65 rows, 50 sweeps, its two seeds) lies
    within 1e-9 of an accept / reject boundary: a float64 implementation takes the same branches as
    this long-double restatement, so the GPU chain can be compared element by element."""
    a = (RC.DEVICE_NU + 1) / 2
    for seed in RC.DEVICE_SEEDS:
        val, attempts, margin = RR.robust_gammas(seed, RC.DEVICE_NU, RC.DEVICE_N, RC.DEVICE_T)
        assert val.shape == (RC.DEVICE_T, RC.DEVICE_N)
        assert margin.min() > R.MARGIN_FLOOR, (seed, margin.min())
        assert attempts.max() < 64 and (val > 0).all()
        # Gamma(a, 1): mean a, variance a; 3250 variates
        assert abs(val.mean() - a) < 5 * np.sqrt(a / val.size)


def test_robust_stream_is_a_function_of_seed_row_and_sweep():
    """g[t, n] depends on (seed, n, t) alone: more rows or sweeps extend the table, another seed or
    another stream word gives other variates."""
    small = RR.robust_gammas(5, 4.0, 7, 3)[0]
    large = RR.robust_gammas(5, 4.0, 9, 6)[0]
    assert np.array_equal(small, large[:3, :7])
    assert not np.array_equal(small, RR.robust_gammas(6, 4.0, 7, 3)[0])
    assert RR.STREAM_ROBUST == int.from_bytes(b"ROBS", "big")
    # not the chain-level gamma stream at the same shape
    assert not np.array_equal(small[:, 0], R.gammas(5, 2.5, 3)[0])


def test_exported_and_argument_errors_come_before_device_work(monkeypatch):
    assert "gibbs_sampler_robust" in pybmc_amd.__all__
    f = pybmc_amd.gibbs_sampler_robust

    def no_device(*a, **kw):
        raise AssertionError("argument errors must be raised before any device work")

    monkeypatch.setattr(_lib, "default_context", no_device)
    y, X = np.zeros(40), np.ones((40, 3))
    prior = (np.zeros(3), np.eye(3), 1.0, 0.02)
    for kw in ({"nu": 0.0}, {"nu": -1.0}, {"nu": float("nan")}, {"burn": -1}, {"n_chains": 0},
               {"n_chains": 2, "seeds": [1, 2, 3]}, {"seeds": [1, 2]}):
        with pytest.raises(ValueError):
            f(y, X, 10, prior, **kw)
    with pytest.raises(ValueError, match="at most 32 columns"):
        f(y, np.ones((40, 33)), 10, (np.zeros(33), np.eye(33), 1.0, 0.02))


def test_header_declares_and_python_binds_the_entry_points():
    with open(HEADER) as fh:
        text = fh.read()
    assert "#define PYBMC_AMD_ABI_VERSION 4" in text          # additive
    m = re.search(r"int bmc_robust_run\(([^;]*)\);", text)
    assert m, "include/pybmc_amd.h does not declare bmc_robust_run"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 13
    assert "nu" in params[1] and "burn" in params[4] and "gl" in params[9]
    assert "row_weight_out" in params[11]
    assert len(_lib.PROTOTYPES["bmc_robust_run"][1]) == len(params)
    m = re.search(r"int bmc_robust_run_device\(([^;]*)\);", text)
    assert m and len(_lib.PROTOTYPES["bmc_robust_run_device"][1]) == len(m.group(1).split(","))
    assert hasattr(_lib.Context, "robust_run") and hasattr(_lib.Context, "robust_run_device")
    lib = _lib.load_library()                                  # exported by the built library
    assert hasattr(lib, "bmc_robust_run") and hasattr(lib, "bmc_robust_run_device")


def test_train_dispatch_and_gaussian_only_methods():
    """The model class: "student_t" is refused by every method whose kernels hard-code the Gaussian
    density, before any device work; `devices` is refused at train()."""
    from pybmc_amd.bmc import BayesianModelCombination
    import pandas as pd
    df = pd.DataFrame({"N": [1, 2, 3], "Z": [1, 1, 2], "a": [1.0, 2.0, 3.0], "b": [1.5, 2.5, 2.0],
                       "truth": [1.2, 2.2, 2.6]})
    bmc = BayesianModelCombination(["a", "b"], {"p": df}, "truth")
    bmc._trained_with = ("student_t", [np.zeros(1), np.eye(1), 1.0, 0.02], 4.0)
    bmc.samples = np.zeros((4, 2))
    bmc.U_hat = np.ones((3, 1))
    bmc.Vt_hat = np.ones((1, 2))
    bmc.S_hat = np.ones(1)
    bmc.centered_experiment_train = np.zeros(3)
    bmc.n_chains = 1
    for call in (bmc.waic, bmc.loo, bmc.loo_predict, bmc.prior_sensitivity,
                 bmc.posterior_predictive_check, bmc.cross_validate, bmc.component_path,
                 lambda: bmc.log_predictive_density(df[["a", "b", "truth"]])):
        with pytest.raises(ValueError, match="supports the Gaussian Gibbs sampler only"):
            call()
    assert bmc._noise_df() == 4.0
    with pytest.raises(ValueError, match="devices"):
        bmc.train({"sampler": "student_t", "devices": [bmc.device + 1], "iterations": 10})
