"""The Student-t (outlier-robust) Gibbs sampler on the MI355X (-m gpu): kernels_robust.hip through
the C ABI and the Python surface, against the long-double numpy reference of
tests/robust_reference.py.

Replay parity bar: 1000 x the deviation of the FLOAT64 numpy reference from the long-double one on
the same case, both relative to each column's scale.  The factor covers a different, tiled summation
order over up to 1237 rows; the chain does not amplify rounding differences (float64 and long-double
replays of one variate set stay within 1.5e-15 of a column's scale over 300 sweeps).  REF_DEV holds
those deviations as measured on the CPU (numpy 300-sweep chains, the max over the three chains):
(samples, row weights) per (N, k, nu).  Measured on one MI355X, the GPU chains deviate from the
long-double reference by 3.1e-16 .. 1.4e-14 (samples) and 3.6e-16 .. 2.2e-15 (weights) over all cases.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from pybmc_amd import _lib

import rng_reference as R
import robust_cases as RC
import robust_reference as RR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

BAR_FACTOR = 1000.0
REF_DEV = {
    (3, 2, 1.5): (8.644e-16, 1.098e-15), (3, 2, 4.0): (7.242e-16, 6.832e-16), (3, 2, 50.0): (5.115e-16, 8.936e-16),
    (65, 1, 1.5): (5.387e-16, 9.479e-16), (65, 1, 4.0): (7.044e-16, 1.158e-15), (65, 1, 50.0): (4.671e-16, 1.861e-15),
    (64, 16, 1.5): (9.736e-15, 1.312e-15), (64, 16, 4.0): (4.228e-15, 1.734e-15), (64, 16, 50.0): (1.417e-15, 1.674e-15),
    (257, 17, 1.5): (6.193e-15, 1.913e-15), (257, 17, 4.0): (4.059e-15, 1.310e-15), (257, 17, 50.0): (2.560e-15, 1.514e-15),
    (629, 3, 1.5): (1.339e-15, 1.101e-15), (629, 3, 4.0): (1.377e-15, 1.306e-15), (629, 3, 50.0): (1.244e-15, 2.166e-15),
    (1237, 5, 1.5): (5.128e-15, 1.685e-15), (1237, 5, 4.0): (4.118e-15, 1.675e-15), (1237, 5, 50.0): (4.030e-15, 1.711e-15),
    (300, 32, 1.5): (1.299e-14, 2.509e-15), (300, 32, 4.0): (8.629e-15, 1.537e-15), (300, 32, 50.0): (5.059e-15, 1.530e-15),
}
# the device-RNG case (65 x 3, 50 sweeps, nu = 4) fed the host-restated variates of its seeds: the
# smaller of the two chains' deviations
DEVICE_DEV = (9.485e-16, 6.709e-16)


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def set_case(ctx, y, X, prior):
    ctx.set_problem(y, X)
    ctx.set_prior(*prior)


@pytest.mark.parametrize("nu", RC.REPLAY_NUS)
@pytest.mark.parametrize("n,k", sorted(RC.REPLAY_CASES))
def test_replay_parity(ctx, n, k, nu):
    y, X, prior = RC.problem(n, k)
    if (n, k) in ((64, 16), (1237, 5)):
        X = np.asfortranarray(X)            # either layout bmc_set_problem accepts
    xi, g, gl = RC.replay_variates(n, k, nu)
    ref, wref = RC.replay_reference(n, k, nu)
    set_case(ctx, y, X, prior)
    out, w, stats = ctx.robust_run(nu, RC.REPLAY_CHAINS, RC.REPLAY_T, xi=xi, g=g, gl=gl)
    assert stats["n_chains"] == RC.REPLAY_CHAINS and stats["launches"] == 1
    dev_s, dev_w = REF_DEV[(n, k, nu)]
    for c in range(RC.REPLAY_CHAINS):
        ds = RC.scaled_deviation(out[c], ref[c])
        dw = RC.weight_deviation(w[c], wref[c])
        print(f"N={n} k={k} nu={nu} chain {c}: samples {ds:.3e} (bar {BAR_FACTOR * dev_s:.3e}), "
              f"weights {dw:.3e} (bar {BAR_FACTOR * dev_w:.3e})")
        assert ds <= BAR_FACTOR * dev_s
        assert dw <= BAR_FACTOR * dev_w


def test_device_rng_is_pinned_to_the_host_streams(ctx):
    y, X, prior = RC.device_problem()
    n, k, T, nu = RC.DEVICE_N, RC.DEVICE_K, RC.DEVICE_T, RC.DEVICE_NU
    set_case(ctx, y, X, prior)
    out, w, _ = ctx.robust_run(nu, len(RC.DEVICE_SEEDS), T, seeds=list(RC.DEVICE_SEEDS))
    for c, seed in enumerate(RC.DEVICE_SEEDS):
        xi = R.normals(seed, T * k).astype(np.float64).reshape(T, k)
        g = R.gammas(seed, (prior[2] + n) / 2, T)[0]
        gl = RR.robust_gammas(seed, nu, n, T)[0]
        ref, wref = RR.chain(y, X, T, prior, nu, xi, g, gl, dtype=np.longdouble)
        ds, dw = RC.scaled_deviation(out[c], ref), RC.weight_deviation(w[c], wref)
        print(f"device RNG chain {c}: samples {ds:.3e}, weights {dw:.3e}")
        assert ds <= BAR_FACTOR * DEVICE_DEV[0]
        assert dw <= BAR_FACTOR * DEVICE_DEV[1]


def test_chain_of_a_large_call_is_its_solo_run(ctx):
    y, X, prior = RC.device_problem()
    set_case(ctx, y, X, prior)
    seeds = np.arange(70, dtype=np.uint64) * 7919 + 3
    out, w, _ = ctx.robust_run(4.0, 70, 50, seeds=seeds)
    again, wagain, _ = ctx.robust_run(4.0, 70, 50, seeds=seeds)
    assert np.array_equal(out, again) and np.array_equal(w, wagain)
    assert np.isfinite(out).all() and np.isfinite(w).all()
    for c in (0, 1, 69):
        solo, wsolo, _ = ctx.robust_run(4.0, 1, 50, seeds=seeds[c:c + 1])
        assert np.array_equal(solo[0], out[c]) and np.array_equal(wsolo[0], w[c])


def test_burn_in_drops_the_leading_sweeps(ctx):
    y, X, prior = RC.device_problem()
    set_case(ctx, y, X, prior)
    full, _, _ = ctx.robust_run(4.0, 1, 87, seeds=[99])
    tail, _, st = ctx.robust_run(4.0, 1, 50, burn=37, seeds=[99])
    assert st["iterations"] == 87
    assert np.array_equal(tail[0], full[0, 37:87])


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
    out, w, st = ctx.robust_run(4.0, n_chains, 12, seeds=seeds)
    assert st["launches"] == 2
    for c in (cap - 1, cap, cap + 1):
        solo, wsolo, _ = ctx.robust_run(4.0, 1, 12, seeds=seeds[c:c + 1])
        assert np.array_equal(solo[0], out[c]) and np.array_equal(wsolo[0], w[c])


def test_planted_outliers_on_the_device():
    """The 200 x 3 planted problem, device RNG, 4 chains: the thresholds of the host test, a smaller
    error of the posterior mean of beta than gibbs_sampler's, rank-normalised R-hat < 1.05."""
    from pybmc_amd import gibbs_sampler, gibbs_sampler_robust
    from pybmc_amd.rankdiag import rank_diagnostics
    y, X, prior, beta_true, idx = RC.planted("200x3")
    n, k = X.shape
    seeds = [41, 42, 43, 44]
    out, lam = gibbs_sampler_robust(y, X, RC.PLANTED_KEEP, prior, 4.0, burn=RC.PLANTED_BURN, n_chains=4,
                                    seeds=seeds, return_row_weights=True)
    assert out.shape == (4, RC.PLANTED_KEEP, k + 1) and lam.shape == (4, n)
    gauss = gibbs_sampler(y, X, RC.PLANTED_BURN + RC.PLANTED_KEEP, prior, n_chains=4, seeds=seeds)
    gauss = gauss[:, RC.PLANTED_BURN:]
    clean = np.setdiff1d(np.arange(n), idx)
    mean_lam = lam.mean(axis=0)
    err_t = np.linalg.norm(out[..., :k].mean(axis=(0, 1)) - beta_true)
    err_g = np.linalg.norm(gauss[..., :k].mean(axis=(0, 1)) - beta_true)
    rhat = np.asarray(rank_diagnostics(out)["r_hat"])
    print(f"planted max {mean_lam[idx].max():.3f}, clean median {np.median(mean_lam[clean]):.3f}, sigma "
          f"{out[..., k].mean():.4f} vs {gauss[..., k].mean():.4f}, beta error {err_t:.4f} vs {err_g:.4f}, "
          f"r_hat max {rhat.max():.4f}")
    assert mean_lam[idx].max() < 0.2
    assert np.median(mean_lam[clean]) > 0.9
    assert out[..., k].mean() < 0.5 * gauss[..., k].mean()
    assert err_t < err_g
    assert np.all(rhat < 1.05)


def test_surface_on_the_standin_dataset():
    from pybmc_amd import BayesianModelCombination, Dataset, gibbs_sampler
    models = ["FRDM", "HFB24", "UNEDF1", "SKM"]
    ds = Dataset(os.path.join(GOLDEN, "dataset_standin.csv"))
    data = ds.load_data(models + ["truth"], keys=["BE"], domain_keys=["N", "Z"])
    train_df, _, _ = ds.split_data(data, "BE", splitting_algorithm="random", train_size=0.6,
                                         val_size=0.2, test_size=0.2)
    b = BayesianModelCombination(models, data, truth_column_name="truth")
    b.orthogonalize("BE", train_df, components_kept=3, method="svd")
    b.train({"sampler": "student_t", "nu": 4, "iterations": 10000, "n_chains": 2, "seeds": [7, 8]})
    n = len(train_df)
    assert b.samples.shape == (20000, 4) and b.n_chains == 2
    assert b.row_weights.shape == (n,) and np.all(b.row_weights > 0)
    assert b._trained_with[0] == "student_t" and b._trained_with[2] == 4.0
    summary = b.summary()
    assert list(summary.index) == ["beta_0", "beta_1", "beta_2", "sigma"] + models
    assert np.isfinite(summary["mean"].to_numpy()).all() and np.all(summary["r_hat"] < 1.1)
    assert list(b.diagnostics().index) == list(summary.index)
    with pytest.raises(ValueError, match="supports the Gaussian Gibbs sampler only"):
        b.waic()
    # predict: W preds' + sigma t with the documented generator
    X = data["BE"][models + ["N", "Z"]].head(37).reset_index(drop=True)
    np.random.seed(2024)
    rndm_m, lo, med, up = b.predict(X)
    np.random.seed(2024)
    seed = int(np.random.randint(0, 2 ** 32, dtype=np.uint64)) << 32 | int(
        np.random.randint(0, 2 ** 32, dtype=np.uint64))
    rng = np.random.Generator(np.random.PCG64(seed))
    theta = rng.choice(np.ascontiguousarray(b.samples), 10000, replace=False)
    preds = X[models].to_numpy(dtype=np.float64)
    t = rng.standard_t(4.0, (10000, preds.shape[0]))
    expect = (theta[:, :3] @ b.Vt_hat + 1.0 / len(models)) @ preds.T + theta[:, 3:4] * t
    assert rndm_m.shape == expect.shape
    assert np.max(np.abs(rndm_m - expect)) <= 1e-12 * np.max(np.abs(expect))
    assert np.all(lo["Predicted_Lower"].to_numpy() <= up["Predicted_Upper"].to_numpy())
    # every other sampler string is still the Gaussian sampler, bit for bit
    b.train({"sampler": "Gibbs_sampling", "iterations": 500, "seeds": [5]})
    assert b.row_weights is None and b._trained_with[0] == "gibbs"
    prior = [np.zeros(3), np.diag(b.S_hat ** 2), 1.0, 0.02]
    direct = gibbs_sampler(b.centered_experiment_train, b.U_hat, 500, prior, seeds=[5])
    assert np.array_equal(b.samples, direct)


def test_refusals_leave_the_context_usable(ctx):
    rng = np.random.default_rng(3)
    y = rng.standard_normal(100)
    X33 = rng.standard_normal((100, 33))
    ctx.set_problem(y, X33)
    ctx.set_prior(np.zeros(33), np.eye(33), 1.0, 0.02)
    with pytest.raises(ValueError, match="1 <= k <= 32"):
        ctx.robust_run(4.0, 1, 10, seeds=[1])
    X = np.ascontiguousarray(X33[:, :3])
    ctx.set_problem(y, X, dtype=np.float32)
    ctx.set_prior(np.zeros(3), np.eye(3), 1.0, 0.02)
    with pytest.raises(ValueError, match="float64"):
        ctx.robust_run(4.0, 1, 10, seeds=[1])
    ctx.set_problem(y, X)
    ctx.set_prior(np.zeros(3), np.eye(3), 1.0, 0.02)
    with pytest.raises(ValueError, match="nu must be positive"):
        ctx.robust_run(-1.0, 1, 10, seeds=[1])
    out, w, st = ctx.robust_run(4.0, 2, 10, seeds=[1, 2])
    assert np.isfinite(out).all() and np.isfinite(w).all() and st["launches"] == 1
