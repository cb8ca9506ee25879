"""CPU checks of the Student-t sampler with nu on a grid: the numpy reference of the step
(tests/robust_nu_reference.py) against the statistics it exists for, the margins the GPU tests rely
on, and the surface (argument errors before any device work, declaration and binding of
bmc_robust_run_nu*)."""
import os
import re

import numpy as np
import pytest

import pybmc_amd
from pybmc_amd import _lib

import rng_reference as R
import robust_cases as RC
import robust_nu_cases as NC
import robust_nu_reference as NR
import robust_reference as RR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "pybmc_amd.h")


def test_grid_of_one_value_is_the_fixed_nu_reference():
    y, X, prior = RC.problem(65, 1)
    T = 40
    xi, g, gl = RR.host_variates(65, 1, T + 5, 4.0, prior[2], seed=3)
    want, wwant = RR.chain(y, X, T, prior, 4.0, xi, g, gl, burn=5)
    got = NR.chain(y, X, T, prior, [4.0], [0.7], 0, xi, g, gl, np.full(T + 5, 0.3), burn=5)
    assert np.array_equal(got["samples"], want) and np.array_equal(got["weights"], wwant)
    assert not got["idx"].any() and np.isfinite(got["tstat"]).all()


@pytest.mark.parametrize("df,lo,hi", ((2.0, 1.3, 3.5), (None, 20.0, np.inf)))
def test_reference_recovers_nu(df, lo, hi):
    """2000 x 3, t_2 or normal noise, the default grid and prior, burn 100, 500 kept sweeps.  Measured
    with these seeds: posterior median 2.08 (t_2 noise; interval asked [1.3, 3.5]) and 26.8 (normal
    noise; asked above 20)."""
    y, X, prior = NC.t_noise_problem(2000, 3, df, seed=5)
    grid, weight, init = NR.default_grid()
    ref = NC.free_reference(y, X, prior, grid, weight, init, 100, 500, seed=9)
    med = float(np.median(grid[ref["idx"]]))
    print(f"noise df {df}: posterior median of nu {med:.3f}")
    assert lo <= med <= hi if np.isfinite(hi) else med > lo


def test_default_grid_matches_the_package():
    from pybmc_amd.inference_utils import robust_nu_prior
    grid, weight, init = robust_nu_prior()
    rg, rw, ri = NR.default_grid()
    assert np.array_equal(grid, rg) and np.allclose(weight, rw, rtol=1e-15) and init == ri
    assert len(grid) == 64 and abs(grid[init] - 4.0) == np.abs(grid - 4.0).min()
    g2, w2, i2 = robust_nu_prior([1.0, 3.0, 9.0], [0.0, 1.0, 1.0], 9.0)
    assert i2 == 2 and np.array_equal(w2, [0.0, 1.0, 1.0])
    assert robust_nu_prior([1.0, 3.9, 9.0], [1.0, 0.0, 1.0])[2] == 0      # nearest 4 of positive weight


def test_stream_is_a_function_of_seed_and_sweep():
    u = NR.nu_uniforms(5, 9)
    assert np.array_equal(u[:4], NR.nu_uniforms(5, 4)) and not np.array_equal(u, NR.nu_uniforms(6, 9))
    assert np.all((u > 0) & (u <= 1))
    assert NR.STREAM_NU == int.from_bytes(b"NUDF", "big")
    assert NR.STREAM_NU not in (R.STREAM_NORMAL, R.STREAM_GAMMA, R.STREAM_PRED_NORMAL, R.STREAM_UNIFORM,
                                RR.STREAM_ROBUST)
    assert not np.array_equal(u, R.uniforms(5, 18)[0::2])               # not the UNIFORM stream


def test_pick_is_the_inverse_cdf():
    with np.errstate(divide="ignore"):
        h, c = np.array([1.0, 2.0, 3.0]), np.log(np.array([0.2, 0.0, 0.8]))
    for u, want in ((0.1, 0), (0.2 - 1e-12, 0), (0.2 + 1e-12, 2), (1.0, 2)):
        assert NR.pick(0.0, h, c, u, np.float64)[0] == want             # never the weight-0 value
    idx, margin = NR.pick(0.0, h, c, 0.5, np.longdouble)
    assert idx == 2 and abs(margin - 0.3) < 1e-15


@pytest.mark.parametrize("n,k", sorted(NC.DEVICE_CASES))
def test_margins_of_the_device_seeds(n, k):
    """No pick and no Marsaglia-Tsang attempt along the reference's own path lies within 1e-9 of a
    boundary, and float64 takes the long-double path: the GPU chain can be compared element by
    element."""
    ld = NC.device_reference(n, k)
    f64 = NC.device_reference(n, k, np.float64)
    for (r, mt), (f, _) in zip(ld, f64):
        assert r["margin"].min() >= R.MARGIN_FLOOR and mt >= R.MARGIN_FLOOR
        assert np.array_equal(r["path"], f["path"]) and len(np.unique(r["path"])) > 1


def test_argument_errors_come_before_device_work(monkeypatch):
    f = pybmc_amd.gibbs_sampler_robust

    def no_device(*a, **kw):
        raise AssertionError("argument errors must be raised before any device work")

    monkeypatch.setattr(_lib, "default_context", no_device)
    y, X = np.zeros(40), np.ones((40, 3))
    prior = (np.zeros(3), np.eye(3), 1.0, 0.02)
    for kw in ({"nu_grid": [2.0, 2.0]}, {"nu_grid": [3.0, 2.0]}, {"nu_grid": np.arange(1.0, 66.0)},
               {"nu_grid": []}, {"nu_grid": [0.0, 1.0]}, {"nu_grid": [1.0, np.inf]},
               {"nu_grid": [1.0, 2.0], "nu_prior": [0.0, 0.0]}, {"nu_grid": [1.0, 2.0], "nu_prior": [1.0]},
               {"nu_grid": [1.0, 2.0], "nu_prior": [-1.0, 1.0]}, {"nu_grid": [1.0, 2.0], "nu_init": 3.0},
               {"nu_grid": [1.0, 2.0], "nu_prior": [0.0, 1.0], "nu_init": 1.0}, {"burn": -1},
               {"n_chains": 2, "seeds": [1]}):
        with pytest.raises(ValueError):
            f(y, X, 10, prior, "estimate", **kw)
    with pytest.raises(ValueError, match="estimate"):
        f(y, X, 10, prior, "guess")
    for kw in ({"nu_grid": [1.0, 2.0]}, {"nu_prior": [1.0]}, {"nu_init": 4.0}, {"return_nu": True}):
        with pytest.raises(ValueError, match='need nu="estimate"'):
            f(y, X, 10, prior, 4.0, **kw)


def test_model_class_surface_of_an_estimated_fit():
    """An estimated fit hands its draws of nu to the predictive noise and to the nu row; a fixed-nu
    fit still reports its number."""
    from pybmc_amd.bmc import BayesianModelCombination
    import pandas as pd
    df = pd.DataFrame({"N": [1, 2, 3], "Z": [1, 1, 2], "a": [1.0, 2.0, 3.0], "b": [1.5, 2.5, 2.0],
                       "truth": [1.2, 2.2, 2.6]})
    bmc = BayesianModelCombination(["a", "b"], {"p": df}, "truth")
    bmc._trained_with = ("student_t", [np.zeros(1), np.eye(1), 1.0, 0.02], "estimate")
    bmc.samples = np.zeros((4, 2))
    bmc.nu_samples = np.array([2.0, 3.0, 2.0, 5.0])
    bmc.n_chains = 2
    assert np.array_equal(bmc._noise_df(), bmc.nu_samples) and bmc._nu_row() == ["nu"]
    assert bmc._nu_chains().shape == (2, 2)
    bmc._trained_with = ("student_t", bmc._trained_with[1], 4.0)
    bmc.nu_samples = None
    assert bmc._noise_df() == 4.0 and bmc._nu_row() == []


def test_scoring_argument_errors_come_before_device_work(monkeypatch):
    from pybmc_amd import scoring

    def no_device(*a, **kw):
        raise AssertionError("argument errors must be raised before any device work")

    monkeypatch.setattr(_lib, "default_context", no_device)
    A, y = np.ones((5, 2)), np.zeros(5)
    s2, s3 = np.ones((30, 3)), np.ones((2, 30, 3))
    for fn in (scoring.pointwise_log_likelihood, scoring.waic, scoring.psis_loo):
        with pytest.raises(ValueError, match="not both"):
            fn(A, y, s2, nu=4.0, nu_draws=np.full(30, 4.0))
        for samples, bad in ((s2, np.full(29, 4.0)), (s2, np.full((1, 30), 4.0)), (s3, np.full(60, 4.0)),
                             (s3, np.full((2, 29), 4.0)), (s3, np.full((2, 30, 1), 4.0))):
            with pytest.raises(ValueError, match="shaped like"):
                fn(A, y, samples, nu_draws=bad)
        for bad in (0.0, -1.0, np.nan, np.inf):
            with pytest.raises(ValueError, match="positive and finite"):
                fn(A, y, s2, nu_draws=np.r_[np.full(29, 4.0), bad])
        with pytest.raises(ValueError, match="at most 4096"):
            fn(A, y, np.ones((5000, 3)), nu_draws=1.0 + np.arange(5000.0))
    vals, idx = scoring._nu_table(np.array([[4.0, 2.0, 4.0, 9.0], [2.0, 2.0, 9.0, 1.0]]), s3[:, :4], 1, 2)
    assert np.array_equal(vals, [1.0, 2.0, 9.0]) and np.array_equal(idx, [1, 2, 1, 0]) and idx.dtype == np.int32


def test_predictive_rows_carry_their_nu():
    from pybmc_amd.sampling_utils import N_PREDICTIVE_DRAWS, _choose
    samples = np.arange(3.0 * 12000).reshape(12000, 3)
    nus = 1.0 + np.arange(12000.0)
    rng = np.random.Generator(np.random.PCG64(7))
    theta, df = _choose(rng, samples, nus)
    assert theta.shape == (N_PREDICTIVE_DRAWS, 3) and df.shape == (N_PREDICTIVE_DRAWS, 1)
    assert np.array_equal(df[:, 0], 1.0 + theta[:, 0] / 3.0)            # each row kept its own nu
    # a fixed nu: the documented stream, choice on the samples alone
    rng = np.random.Generator(np.random.PCG64(7))
    fixed, same = _choose(rng, samples, 4.0)
    want = np.random.Generator(np.random.PCG64(7)).choice(samples, N_PREDICTIVE_DRAWS, replace=False)
    assert same == 4.0 and np.array_equal(fixed, want)
    with pytest.raises(ValueError, match="one value per row"):
        _choose(rng, samples, nus[:5])


def test_header_declares_and_python_binds_the_entry_points():
    with open(HEADER) as fh:
        text = fh.read()
    assert "#define PYBMC_AMD_ABI_VERSION 4" in text          # additive
    m = re.search(r"int bmc_robust_run_nu\(([^;]*)\);", text)
    assert m, "include/pybmc_amd.h does not declare bmc_robust_run_nu"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 20
    assert "nu_grid" in params[1] and "nu_weight" in params[2] and "n_grid" in params[3]
    assert "nu_init" in params[4] and "u_nu" in params[13] and "nu_path" in params[14]
    assert "nu_idx_out" in params[17] and "tstat_out" in params[18]
    assert len(_lib.PROTOTYPES["bmc_robust_run_nu"][1]) == len(params)
    m = re.search(r"int bmc_robust_run_nu_device\(([^;]*)\);", text)
    assert m and len(_lib.PROTOTYPES["bmc_robust_run_nu_device"][1]) == len(m.group(1).split(","))
    assert hasattr(_lib.Context, "robust_run_nu_device")
    lib = _lib.load_library()                                  # exported by the built library
    assert hasattr(lib, "bmc_robust_run_nu") and hasattr(lib, "bmc_robust_run_nu_device")
    for name, scalar in (("bmc_pointwise_loglik_tv", "bmc_pointwise_loglik_t"), ("bmc_psis_loo_tv", "bmc_psis_loo_t")):
        for suffix in ("", "_device"):
            m = re.search(r"int %s%s\(([^;]*)\);" % (name, suffix), text)
            assert m, name + suffix
            params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
            assert "nu_values" in params[10] and "n_values" in params[11] and "nu_index" in params[12]
            assert len(_lib.PROTOTYPES[name + suffix][1]) == len(params)
            assert len(params) == len(_lib.PROTOTYPES[scalar + suffix][1]) + 2   # nu -> three arguments
            assert hasattr(lib, name + suffix) and hasattr(_lib.Context, name[4:] + suffix)
    # the fixed-nu entry points keep their signatures
    m = re.search(r"int bmc_robust_run\(([^;]*)\);", text)
    assert m and len(m.group(1).split(",")) == 13
