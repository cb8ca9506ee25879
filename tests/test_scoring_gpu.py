"""Pointwise log predictive density and WAIC on the MI355X (kernels_waic.hip, pybmc_amd.scoring)
against the dense numpy reference of tests/score_reference.py.

Tolerance: |lppd_i - ref| <= 1e-11 max(1, |ref|); p_waic_i and mean_ll_i 1e-11 relative (+1e-24):
about 100 x the float64 rounding floor of the reference itself (test_scoring_host.py), because the
device's exp / log are not correctly rounded and the MFMA sums in another order."""
import numpy as np
import pytest

import score_reference as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

TOL = 1e-11


def check(got, ref, tag=""):
    d_l = np.abs(got["lppd"] - ref["lppd"]) / np.maximum(1.0, np.abs(ref["lppd"]))
    d_p = np.abs(got["p_waic"] - ref["p_waic"]) / (np.abs(ref["p_waic"]) + 1e-24 / TOL)
    d_m = np.abs(got["mean_ll"] - ref["mean_ll"]) / (np.abs(ref["mean_ll"]) + 1e-24 / TOL)
    print(f"{tag}: lppd {d_l.max():.3e}  p_waic {d_p.max():.3e}  mean_ll {d_m.max():.3e}")
    assert np.isfinite(ref["lppd"]).all() and np.isfinite(ref["p_waic"]).all(), tag
    assert d_l.max() <= TOL, tag
    assert np.all(np.abs(got["p_waic"] - ref["p_waic"]) <= TOL * np.abs(ref["p_waic"]) + 1e-24), tag
    assert np.all(np.abs(got["mean_ll"] - ref["mean_ll"]) <= TOL * np.abs(ref["mean_ll"]) + 1e-24), tag


def plw(*a, **kw):
    from pybmc_amd import pointwise_log_likelihood
    return pointwise_log_likelihood(*a, **kw)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_synthetic_cases_with_a_far_outlier(name):
    A, y, th = R.synth_case(name)
    ref = R.pointwise(A, y, th)
    assert ref["lppd"][0] < -600 and np.isfinite(ref["lppd"][0])   # the running max carries it
    check(plw(A, y, th), ref, name)


@pytest.mark.parametrize("name", ["gibbs_ortho629x3", "gibbs_dense64x8", "gibbs_ragged1237x5"])
def test_golden_chains_as_draws(name):
    g = load_golden(name)
    A, y, th = np.asarray(g["X"], dtype=np.float64), g["y"], g["samples"]
    ref = R.pointwise(A, y, th)
    got = plw(np.asfortranarray(A), y, th)
    check(got, ref, name)
    from pybmc_amd import waic
    w = waic(A, y, th)
    for key, v in R.waic_summary(ref).items():
        assert w[key] == pytest.approx(v, rel=1e-9), key
    if name == "gibbs_ortho629x3":
        assert w["n_high_p"] == 0 and w["p_waic"] == pytest.approx(4.243, abs=5e-4)


random_case = R.random_case


@pytest.mark.parametrize("k", R.SHAPE_K)
def test_shapes_on_both_sides_of_every_rule(k):
    """k across the 4-column MFMA step and the 16-column slab; points and draws across the 64-wide
    tiles (S = 2 and 63 leave lanes without a draw; 4097 with 1000 points takes 13 draw splits,
    the shorter ones a single split); both layouts of A, lda and ldt wider than the rows."""
    from pybmc_amd import _lib
    ctx = _lib.default_context(0)
    for case, n, S, (A, y, th) in R.shape_cases(k):
        ref = R.pointwise(A, y, th)
        pad_a, pad_t = (case % 3) * 2, (case % 2) * 3
        if case % 2:    # column-major, lda = n + pad
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
            got = ctx.pointwise_loglik(buf, n, k, lda, layout, y, tb, S, k + 1 + pad_t)
        check(got, ref, f"k={k} n={n} S={S} layout={layout} lda={lda} ldt={k + 1 + pad_t}")


def test_identical_draws_have_no_variance():
    A, y, th = random_case(300, 7, 2, 5)
    th = np.repeat(th[:1], 1001, axis=0)
    got = plw(A, y, th)
    assert np.all(np.abs(got["lppd"] - got["mean_ll"]) <= 1e-13 * np.maximum(1, np.abs(got["mean_ll"])))
    assert np.all(got["p_waic"] <= 1e-24) and np.all(got["p_waic"] >= 0)
    check({**got, "p_waic": np.zeros(300)}, {**R.pointwise(A, y, th), "p_waic": np.zeros(300)}, "same")


def test_non_finite_values_are_values():
    A, y, th = random_case(200, 5, 700, 9)
    ref = R.pointwise(A, y, th)
    keys = ("lppd", "p_waic", "mean_ll")
    for bad in (np.nan, np.inf):
        A2 = A.copy()
        A2[17, 2] = bad
        got = plw(A2, y, th)
        ok = np.arange(200) != 17
        for key in keys:
            assert np.isnan(got[key][17]), (key, bad)
            np.testing.assert_allclose(got[key][ok], ref[key][ok], rtol=1e-10)
        y2 = y.copy()
        y2[130] = bad
        got = plw(A, y2, th)
        ok = np.arange(200) != 130
        for key in keys:
            assert np.isnan(got[key][130]), (key, bad)
            np.testing.assert_allclose(got[key][ok], ref[key][ok], rtol=1e-10)
    for row, col, val in ((333, 1, np.nan), (699, 5, 0.0), (0, 5, -0.3), (64, 5, np.nan)):
        t2 = th.copy()
        t2[row, col] = val
        got = plw(A, y, t2)
        for key in keys:
            assert np.isnan(got[key]).all(), (key, row, col, val)


def test_deterministic_and_host_equals_device():
    import torch
    from pybmc_amd import _lib
    A, y, th = random_case(500, 12, 9000, 21)
    a = plw(A, y, th)
    b = plw(A, y, th)
    dev = torch.device("cuda", 0)
    wide = torch.full((9000, 20), float("nan"), dtype=torch.float64, device=dev)
    wide[:, :13] = torch.as_tensor(th, device=dev)
    view = wide[:, :13]
    assert view.stride(0) == 20
    c = plw(A, y, view)
    Ad = torch.as_tensor(np.asfortranarray(A).T.copy(), device=dev)   # column-major on the device
    yd = torch.as_tensor(y, device=dev)
    torch.cuda.synchronize()
    ctx = _lib.default_context(0)
    with ctx.lock:
        d = ctx.pointwise_loglik_device(Ad.data_ptr(), 500, 12, 500, _lib.BMC_COL_MAJOR,
                                        yd.data_ptr(), wide.data_ptr(), 9000, 20)
    for key in ("lppd", "p_waic", "mean_ll"):
        assert np.array_equal(a[key], b[key]), key
        assert np.array_equal(a[key], c[key]), key
        assert np.array_equal(a[key], d[key]), key
    check(a, R.pointwise(A, y, th), "determinism case")


def test_pooling_burn_and_thin():
    import torch
    A, y, th = random_case(130, 6, 4 * 1000, 33)
    chains = th.reshape(4, 1000, 7)
    for burn, thin in ((0, 1), (100, 1), (37, 3), (0, 7)):
        ref = R.pointwise(A, y, R.pool(chains, burn, thin))
        check(plw(A, y, chains, burn=burn, thin=thin), ref, f"numpy burn={burn} thin={thin}")
        td = torch.as_tensor(chains, device="cuda:0")
        check(plw(A, y, td, burn=burn, thin=thin), ref, f"torch burn={burn} thin={thin}")
    ref = R.pointwise(A, y, chains[2, 50::4])
    check(plw(A, y, chains[2], burn=50, thin=4), ref, "one chain")
    check(plw(A, y, torch.as_tensor(chains[2], device="cuda:0"), burn=50, thin=4), ref, "one chain, torch")


def test_many_pooled_draws_are_streamed():
    """64 chains x 50 000 draws x 33 columns (845 MB) at 2 000 points: a 51 GB matrix if stored."""
    import torch
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(4)
    rng = np.random.default_rng(4)
    n, k, C, T = 2000, 32, 64, 50000
    A = rng.standard_normal((n, k)) / np.sqrt(k)
    b0 = rng.standard_normal(k)
    y = A @ b0 + 0.1 * rng.standard_normal(n)
    th = torch.randn((C, T, k + 1), generator=g, dtype=torch.float64, device=dev)
    th[..., :k] = th[..., :k] * 0.02 + torch.as_tensor(b0, device=dev)
    th[..., k] = 0.1 * (1.0 + 0.05 * th[..., k])
    got = plw(A, y, th)
    assert all(np.isfinite(v).all() for v in got.values())
    rows = np.arange(0, n, n // 64)[:64]
    host = th.reshape(-1, k + 1).cpu().numpy()
    del th
    ref = R.pointwise(A[rows], y[rows], host, chunk=4)
    check({key: v[rows] for key, v in got.items()}, ref, "64 x 50000 pooled")


def test_scoring_leaves_the_context_alone():
    from gpu_common import gpu_ctx
    from pybmc_amd.synthetic import synth_problem
    ctx = gpu_ctx()
    p = synth_problem(2000, 6, 5, seed=3)
    ctx.set_problem(p["y"], p["X"])
    ctx.set_prior(*p["prior"])
    before, _ = ctx.gibbs_run(2, 400, seeds=[1, 2])
    gen = ctx.problem_generation
    A, y, th = random_case(700, 9, 3000, 2)
    got = ctx.pointwise_loglik(A, 700, 9, 9, 0, y, th, 3000, 10)
    check(got, R.pointwise(A, y, th), "same context")
    # and with the context's own problem and draws
    got = ctx.pointwise_loglik(np.asfortranarray(p["X"]), 2000, 5, 2000, 1, p["y"], before[0], 400, 6)
    check(got, R.pointwise(p["X"], p["y"], before[0]), "own draws")
    after, _ = ctx.gibbs_run(2, 400, seeds=[1, 2])
    assert ctx.problem_generation == gen
    assert before.tobytes() == after.tobytes()


def test_c_abi_refuses_bad_arguments():
    from pybmc_amd import _lib
    ctx = _lib.default_context(0)
    A, y, th = random_case(10, 3, 20, 1)
    for args, msg in (((A, 10, 3, 3, 0, y, th, 1, 4), "n_draws"), ((A, 10, 3, 2, 0, y, th, 20, 4), "lda"),
                      ((A, 10, 3, 9, 1, y, th, 20, 4), "lda"), ((A, 10, 3, 3, 0, y, th, 20, 3), "ldt"),
                      ((A, 0, 3, 3, 0, y, th, 20, 4), "n_points"), ((A, 10, 0, 3, 0, y, th, 20, 4), "k must"),
                      ((A, 10, 257, 257, 0, y, th, 20, 258), "k must"), ((A, 10, 3, 3, 2, y, th, 20, 4), "layout")):
        with pytest.raises(ValueError, match=msg):
            ctx.pointwise_loglik(*args)


# ---- the BayesianModelCombination surface ---------------------------------------------------------
def _fit(kept, sampler="gibbs"):
    from pybmc_amd import BayesianModelCombination
    train, models = R.three_component_frame(400, seed=1)
    b = BayesianModelCombination(models, {"p": train}, truth_column_name="truth")
    with pytest.raises(ValueError, match="orthogonalize"):
        b.waic()
    b.orthogonalize("p", train, components_kept=kept, method="svd")
    with pytest.raises(ValueError, match="train"):
        b.log_predictive_density(train)
    if sampler == "simplex":
        b.train({"iterations": 6000, "sampler": "simplex", "burn": 1000, "stepsize": 0.001})
    else:
        b.train({"iterations": 3000, "burn": 500, "n_chains": 2, "seeds": [1, 2]})
    return b, train


def test_bmc_waic_and_held_out_density():
    b, train = _fit(3)
    w = b.waic()
    ref = R.pointwise(b.U_hat, b.centered_experiment_train, b.samples)
    check({"lppd": w["lppd"], "p_waic": w["p_waic_i"], "mean_ll": w["mean_ll"]}, ref, "bmc.waic")
    for key, v in R.waic_summary(ref).items():
        assert w[key] == pytest.approx(v, rel=1e-9), key
    assert 2.0 < w["p_waic"] < 6.0 and w["n_points"] == 400     # k + 1 = 4 parameters
    # burn drops draws from the start of EACH chain
    s = b.samples.reshape(2, -1, 4)
    wb = b.waic(burn=200)
    check({"lppd": wb["lppd"], "p_waic": wb["p_waic_i"], "mean_ll": wb["mean_ll"]},
          R.pointwise(b.U_hat, b.centered_experiment_train, R.pool(s, 200)), "bmc.waic(burn)")
    # the training frame through the held-out route: the same design matrix up to rounding (the
    # kept rows of Vt are orthogonal to the ones vector)
    lp = b.log_predictive_density(train)
    np.testing.assert_allclose(lp["lppd"], w["lppd"], rtol=1e-9, atol=1e-9)
    assert lp["elpd"] == pytest.approx(float(np.sum(w["lppd"])), rel=1e-9) and lp["n_points"] == 400
    with pytest.raises(ValueError, match="truth"):
        b.log_predictive_density(train.drop(columns=["truth"]))
    with pytest.raises(ValueError, match="DataFrame"):
        b.log_predictive_density(train.values)


def test_held_out_elpd_ranks_components_kept():
    val, _ = R.three_component_frame(200, seed=2)
    e1 = _fit(1)[0].log_predictive_density(val)
    e3 = _fit(3)[0].log_predictive_density(val)
    print(e1["elpd"], e1["se"], e3["elpd"], e3["se"])
    assert e3["elpd"] - e1["elpd"] > max(e3["se"], e1["se"])


def test_simplex_output_is_accepted():
    b, train = _fit(3, sampler="simplex")
    w = b.waic()
    ref = R.pointwise(b.U_hat, b.centered_experiment_train, b.samples)
    check({"lppd": w["lppd"], "p_waic": w["p_waic_i"], "mean_ll": w["mean_ll"]}, ref, "simplex")
