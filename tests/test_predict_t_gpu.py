"""Student-t predictive noise made on the device (-m gpu): Context.predict(nu=) / (nu_draws=),
bmc_predict_t / bmc_predict_tv, and ``noise_source="device"`` of predict() and evaluate().

  1  the noise alone against the restatement of tests/predict_t_reference.py and the CPU build of
     bmc_math.h's student_t_variate (tests/predict_t_host_build.py);
  2  with weights: the device-noise call is the replay of that noise matrix, bit for bit, and lies
     within the bar of the extended-precision reference; bands and coverage are numpy's;
  3  heavy tails through the order statistics;
  4  identities: z[p][s] depends on (seed, p, s, nu_s) alone, the Gaussian call is untouched;
  5  the refusals of the C ABI;
  6  end to end on the planted problem.
"""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

import predict_reference as PR
import predict_t_host_build as H
import predict_t_reference as PT
import robust_reference as RR
from gpu_common import gpu_ctx
from pybmc_amd import _lib, coverage

pytestmark = pytest.mark.gpu

U52 = 2.0 ** -52
PCT = np.arange(0, 101, 5)
Q = (2.5, 50, 97.5, 0, 100, 33.3)


def device_noise(ctx, seed, S, M, nu):
    """Zero weights and preds = 0 isolate the noise: draws / sigma IS the noise matrix (sigma = 2,
    exact).  (S, M) float64."""
    Km, k = 4, 2
    theta = np.column_stack([np.zeros((S, k)), np.full(S, 2.0)])
    dev, _, _ = ctx.predict(np.zeros((M, Km)), theta, np.zeros((k, Km)), seed=seed, q=(), **PT.call_nu(nu, S))
    assert dev.shape == (S, M)
    return dev / 2.0


def weighted_problem(M, Km, k, S):
    rng = np.random.default_rng(M + Km)
    preds = rng.standard_normal((M, Km)) + 3
    theta = np.column_stack([rng.standard_normal((S, k)) * 0.1, rng.uniform(0.5, 1.5, S)])
    Vt = rng.standard_normal((k, Km))
    truth = preds.mean(1) + rng.standard_normal(M)
    return preds, theta, Vt, truth


# ---- 1. the noise alone ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", PT.SEEDS)
@pytest.mark.parametrize("nu", list(PT.NUS) + [PT.CYCLE])
@pytest.mark.parametrize("M,S", [(13, 100), (130, 1000), (96, 10000)])
def test_noise_matrix_is_the_restatement(M, S, nu, seed):
    """No two entries equal, nor equal up to the sign (a counter shared by two entries would make
    that certain); every entry within (T_ACCURACY[nu_s] / 2^-52 + 2) units of 2^-52 |t| of the
    long-double restatement -- the CPU build's recorded worst case plus one ulp each for a device
    sqrt and division; and the bits of the CPU build."""
    ctx = gpu_ctx()
    z = device_noise(ctx, seed, S, M, nu)
    assert np.isfinite(z).all()
    assert len(np.unique(z)) == z.size
    assert len(np.unique(np.abs(z))) == z.size
    ref = PT.noise(seed, S, M, nu)
    units = np.abs(z.astype(PT.LD) - ref) / np.abs(ref) / U52
    bar = PT.accuracy(nu, S) / U52 + 2.0
    cpu = H.noise(seed, S, M, nu)
    differ = int((z != cpu).sum())
    i = np.unravel_index(int((units / bar).argmax()), units.shape)
    print(f"t noise {S} x {M} nu {nu} seed {seed}: worst {float(units.max()):.3f} units of 2^-52 |t|; "
          f"worst against its bar {float(units[i]):.3f} of {float(bar[i[0], 0]):.1f}; "
          f"{differ} of {z.size} entries differ from the CPU build")
    assert np.all(units <= bar), (i, float(units[i]))
    assert differ == 0


# ---- 2. with weights ------------------------------------------------------------------------------
@pytest.mark.parametrize("nu", [4.0, PT.CYCLE])
@pytest.mark.parametrize("M,Km,k,S", [(1, 2, 1, 64), (13, 6, 3, 100), (65, 5, 3, 1000), (130, 33, 32, 10000),
                                      (7, 257, 9, 4097)])
def test_device_noise_call_is_the_replay_of_its_noise(M, Km, k, S, nu):
    ctx = gpu_ctx()
    preds, theta, Vt, truth = weighted_problem(M, Km, k, S)
    for seed in PT.SEEDS:
        Z = device_noise(ctx, seed, S, M, nu)
        dev, bands, cov = ctx.predict(preds, theta, Vt, seed=seed, q=Q, truth=truth, cov_percentiles=PCT,
                                      **PT.call_nu(nu, S))
        assert dev.shape == (S, M)
        rep, _, _ = ctx.predict(preds, theta, Vt, noise=Z, q=Q)
        assert np.array_equal(dev, rep), float(np.abs(dev - rep).max())
        ref, bar = PR.predictive_reference(preds, theta, Vt, Z)
        err = np.abs(dev.astype(PR.np.longdouble) - ref)
        print(f"({M}, {Km}, {k}, {S}) nu {nu} seed {seed}: worst error / bar {float((err / bar).max()):.3f}")
        assert np.all(err <= bar)
        assert np.array_equal(bands, np.percentile(dev, Q, axis=0))
        assert coverage(PCT, dev, pd.DataFrame({"truth": truth}), "truth") == cov


# ---- 3. heavy tails through the order statistics ---------------------------------------------------
@pytest.mark.parametrize("nu", [1.5, 0.5])
@pytest.mark.parametrize("S", [2048, 10000, 16384])
def test_heavy_tails_through_the_order_statistics(S, nu):
    """A range stretched by far outliers puts more than SEL_CAP draws into a requested bin: such
    points go from the selection to the sort.  Bands and coverage stay numpy's on the returned
    draws."""
    ctx = gpu_ctx()
    M = 70
    preds, theta, Vt, truth = weighted_problem(M, 5, 3, S)
    dev, bands, cov = ctx.predict(preds, theta, Vt, seed=PT.SEEDS[0], q=Q, truth=truth, cov_percentiles=PCT,
                                  nu=nu)
    assert dev.shape == (S, M) and np.isfinite(dev).all()
    ranks = PR.requested_ranks(S, Q, PCT)
    routes = [PR.selection_route(dev[:, p], ranks) for p in range(M)]
    print(f"nu {nu} S {S}: max |draw| {np.abs(dev).max():.3e}; routes "
          + ", ".join(f"{r} {routes.count(r)}" for r in sorted(set(routes))))
    assert np.array_equal(bands, np.percentile(dev, Q, axis=0))
    assert coverage(PCT, dev, pd.DataFrame({"truth": truth}), "truth") == cov


# ---- 4. identities ---------------------------------------------------------------------------------
def test_identities():
    ctx = gpu_ctx()
    M, Km, k, S = 13, 6, 3, 100
    preds, theta, Vt, _ = weighted_problem(M, Km, k, S)
    seed = PT.SEEDS[1]
    gauss_before, gb, _ = ctx.predict(preds, theta, Vt, seed=seed)
    one, b1, _ = ctx.predict(preds, theta, Vt, seed=seed, nu=4.0)
    # predict_draws("F") and predict_timing() after a t call
    assert np.array_equal(ctx.predict_draws("F"), one)
    assert ctx.predict_draws("F").flags["F_CONTIGUOUS"]
    tm = ctx.predict_timing()
    assert all(np.isfinite(v) and v >= 0 for v in tm.values()) and tm["gemm_ms"] > 0
    # one repeated value per draw gives the bits of nu=
    rep, b2, _ = ctx.predict(preds, theta, Vt, seed=seed, nu_draws=np.full(S, 4.0))
    assert np.array_equal(rep, one) and np.array_equal(b1, b2)
    col, _, _ = ctx.predict(preds, theta, Vt, seed=seed, nu_draws=np.full((S, 1), 4.0))
    assert np.array_equal(col, one)
    # changing nu_draws[s] changes column (draw) s only
    nus = np.full(S, 4.0)
    nus[70] = 1.5
    moved = ctx.predict(preds, theta, Vt, seed=seed, nu_draws=nus)[0] != one
    assert moved[70].all() and not np.delete(moved, 70, axis=0).any()
    # the first 7 points of a 13-point call are the 7-point call
    cyc = PT.nu_of_draws(PT.CYCLE, S)
    d13 = ctx.predict(preds, theta, Vt, seed=seed, nu_draws=cyc)[0]
    d7 = ctx.predict(preds[:7], theta, Vt, seed=seed, nu_draws=cyc)[0]
    assert np.array_equal(d13[:, :7], d7)
    # the same seed gives the same draws, another seed others
    assert np.array_equal(ctx.predict(preds, theta, Vt, seed=seed, nu=4.0)[0], one)
    other = ctx.predict(preds, theta, Vt, seed=seed + 1, nu=4.0)[0]
    assert not (other == one).any()
    # t noise is not the Gaussian call's noise, and the Gaussian call keeps its bits
    assert not (one == gauss_before).any()
    gauss_after, ga, _ = ctx.predict(preds, theta, Vt, seed=seed)
    assert np.array_equal(gauss_before, gauss_after) and np.array_equal(gb, ga)


# ---- 5. C-ABI refusals ------------------------------------------------------------------------------
def test_c_abi_refusals_leave_the_context_usable():
    ctx = gpu_ctx()
    lib, h = ctx._lib, ctx._h
    M, Km, k, S = 5, 3, 2, 64
    preds, theta, Vt, _ = weighted_problem(M, Km, k, S)
    qi, qg = _lib.order_stat_plan(S, (50,))
    bands = np.empty((1, M))
    D = _lib._dptr
    i32p = C.POINTER(C.c_int32)

    def t_call(nu, preds=preds, S=S):
        return lib.bmc_predict_t(h, D(preds), M, Km, D(theta), S, k, D(Vt), 3, qi.ctypes.data_as(i32p), D(qg),
                                 1, None, None, None, 0, None, D(bands), None, nu)

    def tv_call(nus, S=S):
        return lib.bmc_predict_tv(h, D(preds), M, Km, D(theta), S, k, D(Vt), 3, qi.ctypes.data_as(i32p),
                                  D(qg), 1, None, None, None, 0, None, D(bands), None, D(nus))

    good = np.full(S, 4.0)
    einval = 1
    for nu in (0.05, 0.0, -4.0, float("inf"), float("nan")):
        assert t_call(nu) == einval, nu
        assert b"nu" in lib.bmc_last_error(h)
        assert t_call(4.0) == 0
        bad = good.copy()
        bad[S - 1] = nu
        assert tv_call(bad) == einval, nu
        assert tv_call(good) == 0
    assert tv_call(None) == einval
    assert tv_call(good) == 0
    # everything bmc_predict refuses: no preds, no draws, too many draws
    assert t_call(4.0, preds=None) == einval
    assert t_call(4.0, S=0) == einval and tv_call(good, S=0) == einval
    assert t_call(4.0, S=16385) == einval
    assert t_call(4.0) == 0 and np.isfinite(bands).all()
    # and through the binding: ValueError
    with pytest.raises(ValueError):
        ctx._check(t_call(0.05))
    assert ctx.predict(preds, theta, Vt, seed=3, nu=0.06)[0].shape == (S, M)


# ---- 6. end to end -----------------------------------------------------------------------------------
def planted_bmc(n_points):
    """A BayesianModelCombination standing on robust_reference.planted_problem(200, 3, 0.05, 11), as
    tests/test_ppc_t_gpu.py builds it, with a property of ``n_points`` rows to predict and evaluate."""
    from pybmc_amd import BayesianModelCombination
    y, X, prior, _, _ = RR.planted_problem(200, 3, 0.05, 11)
    rng = np.random.default_rng(8)
    models = ["a", "b", "c", "d"]
    df = pd.DataFrame(rng.standard_normal((n_points, 4)) + 3, columns=models)
    df["truth"] = 0.0     # (set from the fit, below: evaluate() needs a truth the fit can cover)
    df["N"] = np.arange(n_points)
    b = BayesianModelCombination(models, {"p": df}, truth_column_name="truth")
    b.U_hat = X
    b.S_hat = np.sqrt(np.diag(prior[1]))
    b.Vt_hat = np.random.default_rng(9).standard_normal((3, 4))
    b.centered_experiment_train = y
    b._predictions_mean_train = np.zeros(200)
    b.current_property = "p"
    return b, df


@pytest.mark.parametrize("nu", [4, "estimate"])
def test_predict_and_evaluate_with_device_noise(nu):
    b, df = planted_bmc(37)
    models = b.models
    b.train({"sampler": "student_t", "nu": nu, "iterations": 3000, "n_chains": 4, "seeds": [21, 22, 23, 24]})
    assert b.samples.shape == (12000, 4)
    X = df[models + ["N"]]
    preds = X[models].to_numpy(dtype=np.float64)
    np.random.seed(2024)
    dev, lo, med, up = b.predict(X, noise_source="device")
    np.random.seed(2024)
    host, _, _, _ = b.predict(X)
    assert dev.shape == (10000, 37) and np.isfinite(dev).all()
    lo, med, up = (f[c].to_numpy() for f, c in ((lo, "Predicted_Lower"), (med, "Predicted_Median"),
                                                (up, "Predicted_Upper")))
    assert np.all(lo <= med) and np.all(med <= up)
    # the same choice of rows on both paths
    np.random.seed(2024)
    seed = int(np.random.randint(0, 2 ** 32, dtype=np.uint64)) << 32 | int(
        np.random.randint(0, 2 ** 32, dtype=np.uint64))
    rng = np.random.Generator(np.random.PCG64(seed))
    if nu == "estimate":
        both = rng.choice(np.column_stack([np.ascontiguousarray(b.samples), b.nu_samples]), 10000, replace=False)
        theta, df_t = np.ascontiguousarray(both[:, :-1]), both[:, -1:]
        print(f"estimated nu of the chosen rows: {df_t.min():.3f} .. {df_t.max():.3f}")
    else:
        theta, df_t = rng.choice(np.ascontiguousarray(b.samples), 10000, replace=False), 4.0
    t = rng.standard_t(df_t, (10000, 37))
    mean = (theta[:, :3] @ b.Vt_hat + 1.0 / len(models)) @ preds.T
    # the default keyword: the formula tests/test_robust_gpu.py asserts
    expect = mean + theta[:, 3:4] * t
    assert np.max(np.abs(host - expect)) <= 1e-12 * np.max(np.abs(expect))
    # the device path: its noise recovered as in part 1, the noiseless part is the host path's
    Z = device_noise(_lib.default_context(0), seed, 10000, 37, df_t.reshape(-1) if nu == "estimate" else 4.0)
    scale = max(1.0, np.abs(dev).max(), np.abs(host).max())
    d_mean, h_mean = dev - theta[:, 3:4] * Z, host - theta[:, 3:4] * t
    print(f"nu {nu}: noiseless parts differ by {np.abs(d_mean - h_mean).max():.3e}, scale {scale:.3e}")
    assert np.abs(d_mean - h_mean).max() <= 1e-12 * scale
    assert np.abs(d_mean - mean).max() <= 1e-12 * scale
    assert not np.array_equal(dev, host)
    # a truth near the fit's own prediction (within about one sigma): the 100 % interval, the range
    # of 10 000 draws, covers every point
    off = 0.1 * np.random.default_rng(10).standard_normal(37)
    b.data_dict["p"]["truth"] = mean.mean(axis=0) + off
    cov = b.evaluate(noise_source="device")
    print(f"nu {nu}: coverage " + " ".join(f"{c:.0f}" for c in cov))
    assert len(cov) == 21 and np.all(np.diff(cov) >= 0) and cov[0] == 0 and cov[-1] == 100
