"""The Student-t sampler with nu on a grid on the MI355X (-m gpu): robust_chain_kernel<KC, true>
through bmc_robust_run_nu and the Python surface, against the long-double numpy reference of
tests/robust_nu_reference.py.

Parity bar, the rule of test_robust_gpu.py: BAR_FACTOR = 1000 x the deviation of the FLOAT64 numpy
restatement from the long-double one on the same case.  REF_DEV holds those deviations as measured on
the CPU (300-sweep chains on the forced paths, the max over the three chains): (samples relative to
each column's scale, row weights relative to the largest, T_t relative to n) per (N, k).  The discrete
picks are compared exactly: the test first asserts on the reference alone that no pick lies within
MARGIN_FLOOR of a boundary.  Measured on one MI355X over the five replay cases, the GPU chains deviate
from the long-double reference by 5.0e-16 .. 3.2e-15 (samples), 3.3e-16 .. 1.3e-15 (weights) and
2.8e-16 .. 1.1e-15 (T_t); the device-RNG chains by up to 1.0e-14 / 1.1e-15 / 5.7e-16.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from pybmc_amd import _lib

import rng_reference as R
import robust_cases as RC
import robust_nu_cases as NC
import robust_nu_reference as NR
import robust_reference as RR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

BAR_FACTOR = 1000.0
REF_DEV = {
    (3, 2): (1.056e-15, 7.757e-16, 1.178e-15),
    (65, 1): (5.031e-16, 1.282e-15, 3.605e-16),
    (257, 17): (3.872e-15, 1.508e-15, 9.025e-16),
    (64, 16): (4.014e-15, 1.163e-15, 8.700e-16),
    (300, 8): (8.135e-15, 1.421e-15, 4.593e-16),
}
NU_KW = dict(nu_grid=NC.GRID, nu_weight=NC.WEIGHT, nu_init=NC.NU_INIT)


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def set_case(ctx, y, X, prior):
    ctx.set_problem(y, X)
    ctx.set_prior(*prior)


def assert_parity(label, n, k, out, w, ts, ref):
    dev_s, dev_w, dev_t = REF_DEV[(n, k)]
    ds = RC.scaled_deviation(out, ref["samples"])
    dw = RC.weight_deviation(w, ref["weights"])
    dt = NC.tstat_deviation(ts, ref["tstat"], n)
    print(f"{label}: samples {ds:.3e} (bar {BAR_FACTOR * dev_s:.3e}), weights {dw:.3e} (bar "
          f"{BAR_FACTOR * dev_w:.3e}), T {dt:.3e} (bar {BAR_FACTOR * dev_t:.3e})")
    assert ds <= BAR_FACTOR * dev_s
    assert dw <= BAR_FACTOR * dev_w
    assert dt <= BAR_FACTOR * dev_t


@pytest.mark.parametrize("n,k", NC.REPLAY_CASES)
def test_forced_path_replay_parity(ctx, n, k):
    y, X, prior = NC.problem(n, k)
    paths, xi, g, gl, u = NC.replay_inputs(n, k)
    ref = NC.replay_reference(n, k)
    for c in range(NC.CHAINS):      # the condition the exact comparison of the picks rests on
        assert ref[c]["margin"].min() >= R.MARGIN_FLOOR
        assert {0, len(NC.GRID) - 1} <= set(paths[c].tolist()) and np.count_nonzero(np.diff(paths[c])) > 50
    set_case(ctx, y, X, prior)
    out, w, idx, ts, stats = ctx.robust_run(None, NC.CHAINS, NC.T, xi=xi, g=g, gl=gl, u_nu=u, nu_path=paths,
                                            want_tstat=True, **NU_KW)
    assert stats["n_chains"] == NC.CHAINS and stats["launches"] == 1
    for c in range(NC.CHAINS):
        assert_parity(f"N={n} k={k} chain {c}", n, k, out[c], w[c], ts[c], ref[c])
        assert np.array_equal(idx[c], ref[c]["idx"])


@pytest.mark.parametrize("n,k", sorted(NC.DEVICE_CASES))
def test_device_rng_is_pinned_to_the_host_streams(ctx, n, k):
    y, X, prior = NC.problem(n, k)
    seeds = NC.DEVICE_CASES[(n, k)]
    ref = NC.device_reference(n, k)
    for r, mt_margin in ref:
        assert r["margin"].min() >= R.MARGIN_FLOOR and mt_margin >= R.MARGIN_FLOOR
    set_case(ctx, y, X, prior)
    out, w, idx, ts, _ = ctx.robust_run(None, len(seeds), NC.T, seeds=list(seeds), want_tstat=True, **NU_KW)
    for c, (r, _) in enumerate(ref):
        assert np.array_equal(idx[c], r["idx"]), f"chain {c}: the index path left the reference's"
        assert len(np.unique(idx[c])) > 1
        assert_parity(f"device RNG N={n} k={k} chain {c}", n, k, out[c], w[c], ts[c], r)


@pytest.mark.parametrize("n,k", ((3, 2), (300, 8), (64, 16), (257, 17)))
def test_grid_of_one_value_is_the_fixed_nu_run(ctx, n, k):
    y, X, prior = NC.problem(n, k)
    set_case(ctx, y, X, prior)
    seeds = [11, 12, 13]
    fixed, wfixed, _ = ctx.robust_run(4.0, 3, 120, burn=7, seeds=seeds)
    out, w, idx, ts, _ = ctx.robust_run(None, 3, 120, burn=7, seeds=seeds, nu_grid=[4.0], nu_weight=[1.0],
                                        nu_init=0, want_tstat=True)
    assert np.array_equal(out, fixed) and np.array_equal(w, wfixed)
    assert np.array_equal(idx, np.zeros((3, 120), dtype=np.int32)) and np.isfinite(ts).all()
    # and on replayed variates
    T = 60
    xi, g, gl = (np.stack(p) for p in zip(*[RR.host_variates(n, k, T, 4.0, prior[2], seed=c) for c in range(3)]))
    fixed, wfixed, _ = ctx.robust_run(4.0, 3, T, xi=xi, g=g, gl=gl)
    out, w, idx, _, _ = ctx.robust_run(None, 3, T, xi=xi, g=g, gl=gl, u_nu=np.full((3, T), 0.5),
                                       nu_path=np.zeros((3, T), dtype=np.int32), nu_grid=[4.0],
                                       nu_weight=[2.5], nu_init=0)
    assert np.array_equal(out, fixed) and np.array_equal(w, wfixed) and not idx.any()


def test_chain_of_a_larger_call_is_its_solo_run(ctx):
    y, X, prior = RC.device_problem()
    set_case(ctx, y, X, prior)
    seeds = np.arange(5, dtype=np.uint64) * 7919 + 3
    out, w, idx, ts, _ = ctx.robust_run(None, 5, 80, seeds=seeds, want_tstat=True, **NU_KW)
    again = ctx.robust_run(None, 5, 80, seeds=seeds, want_tstat=True, **NU_KW)
    for a, b in zip((out, w, idx, ts), again):
        assert np.array_equal(a, b)
    assert np.isfinite(out).all() and np.isfinite(w).all() and np.isfinite(ts).all()
    assert idx.min() >= 0 and idx.max() < len(NC.GRID) and len(np.unique(idx)) > 1
    for c in (0, 2, 4):
        solo = ctx.robust_run(None, 1, 80, seeds=seeds[c:c + 1], want_tstat=True, **NU_KW)
        for a, b in zip((out, w, idx, ts), solo):
            assert np.array_equal(a[c], b[0])


def test_burn_in_drops_the_leading_sweeps(ctx):
    y, X, prior = RC.device_problem()
    set_case(ctx, y, X, prior)
    full, _, idx, ts, _ = ctx.robust_run(None, 1, 87, seeds=[99], want_tstat=True, **NU_KW)
    tail, _, tidx, tts, st = ctx.robust_run(None, 1, 50, burn=37, seeds=[99], want_tstat=True, **NU_KW)
    assert st["iterations"] == 87
    assert np.array_equal(tail[0], full[0, 37:87])
    assert np.array_equal(tidx[0], idx[0, 37:87]) and np.array_equal(tts[0], ts[0, 37:87])


def test_chains_on_both_sides_of_a_launch_boundary(ctx, tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "a host C++ compiler is required"
    exe = str(tmp_path / "robust_plan_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(HERE, "robust_plan_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cap = int(subprocess.run([exe, "launches", "1"], capture_output=True, text=True,
                             check=True).stdout.split("|")[0])
    n_chains = cap + 2
    y, X, prior = RC.device_problem()
    set_case(ctx, y, X, prior)
    seeds = np.arange(n_chains, dtype=np.uint64) + 1000
    out, w, idx, _, st = ctx.robust_run(None, n_chains, 12, seeds=seeds, **NU_KW)
    assert st["launches"] == 2
    for c in (cap - 1, cap, cap + 1):
        solo, wsolo, isolo, _, _ = ctx.robust_run(None, 1, 12, seeds=seeds[c:c + 1], **NU_KW)
        assert np.array_equal(solo[0], out[c]) and np.array_equal(wsolo[0], w[c])
        assert np.array_equal(isolo[0], idx[c])


def test_planted_outliers_on_the_device():
    """The 200 x 3 planted problem, device RNG, 4 chains, the default grid and prior: rank-normalised
    R-hat of nu below the 1.05 of test_robust_gpu.py's columns, and the posterior median of nu inside
    the central 98 % interval of a float64 reference chain (numpy variates, same burn and length)."""
    from pybmc_amd import gibbs_sampler_robust
    from pybmc_amd.rankdiag import rank_diagnostics
    y, X, prior, _, _ = RC.planted("200x3")
    n, k = X.shape
    out, lam, nus = gibbs_sampler_robust(y, X, RC.PLANTED_KEEP, prior, "estimate", burn=RC.PLANTED_BURN,
                                         n_chains=4, seeds=[41, 42, 43, 44], return_row_weights=True,
                                         return_nu=True)
    assert out.shape == (4, RC.PLANTED_KEEP, k + 1) and lam.shape == (4, n)
    assert nus.shape == (4, RC.PLANTED_KEEP)
    grid, weight, init = NR.default_grid()
    assert np.isin(nus, grid).all()
    ref = NC.free_reference(y, X, prior, grid, weight, init, RC.PLANTED_BURN, RC.PLANTED_KEEP, seed=77)
    lo, hi = np.quantile(grid[ref["idx"]], [0.01, 0.99])
    rhat = float(np.asarray(rank_diagnostics(nus[..., None])["r_hat"])[0])
    med = float(np.median(nus))
    print(f"nu: median {med:.3f}, reference 98 % interval [{lo:.3f}, {hi:.3f}], r_hat {rhat:.4f}")
    assert rhat < 1.05
    assert lo <= med <= hi


def test_surface_on_the_standin_dataset():
    from pybmc_amd import BayesianModelCombination, Dataset
    models = ["FRDM", "HFB24", "UNEDF1", "SKM"]
    ds = Dataset(os.path.join(GOLDEN, "dataset_standin.csv"))
    data = ds.load_data(models + ["truth"], keys=["BE"], domain_keys=["N", "Z"])
    train_df, _, _ = ds.split_data(data, "BE", splitting_algorithm="random", train_size=0.6,
                                   val_size=0.2, test_size=0.2)
    b = BayesianModelCombination(models, data, truth_column_name="truth")
    b.orthogonalize("BE", train_df, components_kept=3, method="svd")
    grid = np.geomspace(1.0, 60.0, 24)
    b.train({"sampler": "student_t", "nu": "estimate", "nu_grid": grid, "nu_prior": np.ones(24),
             "iterations": 6000, "n_chains": 2, "seeds": [7, 8]})
    assert b.samples.shape == (12000, 4) and b.n_chains == 2
    assert b.nu_samples.shape == (12000,) and np.isin(b.nu_samples, grid).all()
    assert b.row_weights.shape == (len(train_df),) and np.all(b.row_weights > 0)
    assert b._trained_with[0] == "student_t" and b._trained_with[2] == "estimate"
    summary = b.summary()
    assert list(summary.index) == ["beta_0", "beta_1", "beta_2", "sigma", "nu"] + models
    assert np.isfinite(summary["mean"].to_numpy()).all()
    assert abs(summary.loc["nu", "mean"] - b.nu_samples.mean()) <= 1e-9 * b.nu_samples.mean()
    assert list(b.diagnostics().index) == list(summary.index)
    # predict: W preds' + sigma_s t_{nu_s}, rows chosen from samples with nu appended
    X = data["BE"][models + ["N", "Z"]].head(37).reset_index(drop=True)
    np.random.seed(2024)
    rndm_m, lo, med, up = b.predict(X)
    np.random.seed(2024)
    seed = int(np.random.randint(0, 2 ** 32, dtype=np.uint64)) << 32 | int(
        np.random.randint(0, 2 ** 32, dtype=np.uint64))
    rng = np.random.Generator(np.random.PCG64(seed))
    both = rng.choice(np.column_stack([b.samples, b.nu_samples]), 10000, replace=False)
    theta, df = both[:, :4], both[:, 4:]
    preds = X[models].to_numpy(dtype=np.float64)
    t = rng.standard_t(df, (10000, preds.shape[0]))
    expect = (theta[:, :3] @ b.Vt_hat + 1.0 / len(models)) @ preds.T + theta[:, 3:4] * t
    assert rndm_m.shape == expect.shape
    assert np.max(np.abs(rndm_m - expect)) <= 1e-12 * np.max(np.abs(expect))
    assert np.all(lo["Predicted_Lower"].to_numpy() <= up["Predicted_Upper"].to_numpy())
    cov = b.evaluate()
    assert len(cov) == 21 and cov[0] == 0 and cov[-1] <= 100
    # a fixed nu afterwards is the fixed-nu fit: no nu row, no nu draws
    b.train({"sampler": "student_t", "nu": 4, "iterations": 500, "seeds": [5]})
    assert b.nu_samples is None and b._noise_df() == 4.0
    assert "nu" not in b.summary().index


def test_refusals_leave_the_context_usable(ctx):
    y, X, prior = RC.device_problem()
    set_case(ctx, y, X, prior)
    ok = dict(nu_grid=[2.0, 4.0], nu_weight=[1.0, 1.0], nu_init=0)
    for bad, match in ((dict(ok, nu_grid=[4.0, 2.0]), "strictly increasing"),
                       (dict(ok, nu_grid=[0.0, 2.0]), "positive and finite"),
                       (dict(ok, nu_weight=[0.0, 0.0]), "at least one"),
                       (dict(ok, nu_weight=[-1.0, 1.0]), "non-negative"),
                       (dict(ok, nu_init=2), "must index"),
                       (dict(ok, nu_weight=[0.0, 1.0]), "positive prior weight"),
                       (dict(nu_grid=np.arange(1.0, 66.0), nu_weight=np.ones(65), nu_init=0), "n_grid <= 64")):
        with pytest.raises(ValueError, match=match):
            ctx.robust_run(None, 1, 10, seeds=[1], **bad)
    T = 10
    xi, g, gl = RR.host_variates(RC.DEVICE_N, RC.DEVICE_K, T, 4.0, prior[2], seed=1)
    with pytest.raises(ValueError, match="nu_path must index"):
        ctx.robust_run(None, 1, T, xi=xi, g=g, gl=gl, u_nu=np.full(T, 0.5), nu_path=np.full(T, 2), **ok)
    out, w, idx, _, st = ctx.robust_run(None, 2, 10, seeds=[1, 2], **ok)
    assert np.isfinite(out).all() and np.isfinite(w).all() and st["launches"] == 1
    assert idx.min() >= 0 and idx.max() <= 1
