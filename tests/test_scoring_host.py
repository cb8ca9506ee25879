"""CPU checks of the scoring feature (pybmc_amd.scoring, kernels_waic.hip's split plan):
the numpy reference against extended precision, the reference's summaries on the golden chains,
the split plan of bmc_plan.h (g++ builds tests/score_plan_check.cpp), argument validation."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import score_reference as R
from conftest import load_golden

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_reference_rounding_floor(name):
    """float64 reference, dense and in 64-draw-tile online order, against np.longdouble: the floor
    the device tolerance (1e-11) is derived from.  Measured: lppd 8.3e-14 abs, p_waic 1.4e-14 rel."""
    A, y, th = R.synth_case(name)
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("no extended precision on this platform")
    ext = R.pointwise(A, y, th, dtype=np.longdouble)
    assert np.isfinite(np.asarray(ext["lppd"], dtype=np.float64)).all()
    assert float(ext["lppd"][0]) < -600    # the 40-sigma point
    for form in (R.pointwise(A, y, th), R.pointwise_online(A, y, th)):
        e_l = np.abs(form["lppd"] - ext["lppd"]).max()
        e_p = (np.abs(form["p_waic"] - ext["p_waic"]) / ext["p_waic"]).max()
        e_m = (np.abs(form["mean_ll"] - ext["mean_ll"]) / np.abs(ext["mean_ll"])).max()
        print(name, float(e_l), float(e_p), float(e_m))
        assert e_l < 5e-13 and e_p < 1e-13 and e_m < 1e-13


def golden_draws(name):
    g = load_golden(name)
    return np.asarray(g["X"], dtype=np.float64), g["y"], g["samples"]


def test_reference_summaries_on_golden_chains():
    """The unmodified reference's own chains as posterior draws: pins the summaries."""
    A, y, th = golden_draws("gibbs_ortho629x3")
    pw = R.pointwise(A, y, th)
    s = R.waic_summary(pw)
    assert s["n_points"] == 629 and s["n_high_p"] == 0
    assert s["p_waic"] == pytest.approx(4.243, abs=5e-4)      # k + 1 = 4 parameters
    assert s["elpd_waic"] == pytest.approx(522.75, abs=5e-3)
    assert s["se"] == pytest.approx(16.81, abs=5e-3)
    assert s["waic"] == -2.0 * s["elpd_waic"]
    A, y, th = golden_draws("gibbs_dense64x8")
    s8 = R.waic_summary(R.pointwise(A, y, th))
    assert s8["p_waic"] == pytest.approx(6.65, abs=5e-3) and s8["n_high_p"] == 3
    # the package's host summaries are the reference's, to 1e-9 relative
    from pybmc_amd import scoring
    mine = scoring.waic_summary(pw["lppd"], pw["p_waic"])
    for key, v in s.items():
        assert mine[key] == pytest.approx(v, rel=1e-9), key
    e = scoring.elpd_summary(pw["lppd"])
    for key, v in R.elpd_summary(pw).items():
        assert e[key] == pytest.approx(v, rel=1e-9), key


def test_online_form_matches_dense_on_golden():
    A, y, th = golden_draws("gibbs_dense64x8")
    a, b = R.pointwise(A, y, th), R.pointwise_online(A, y, th)
    for key in a:
        np.testing.assert_allclose(b[key], a[key], rtol=1e-12, atol=1e-13)


# ---- split plan ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is required")
    exe = tmp_path_factory.mktemp("score_plan") / "score_plan_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                        os.path.join(HERE, "score_plan_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def plan(exe, n, S, k, n_cu=256):
    r = subprocess.run([exe, "plan", str(n), str(S), str(k), str(n_cu)], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    return dict((kv.split("=")[0], int(kv.split("=")[1])) for kv in r.stdout.split())


def test_split_plan_named_shapes(plan_exe):
    c1 = plan(plan_exe, 377, 50000, 3)
    assert c1["point_tiles"] == 6 and c1["draw_tiles"] == 782 and c1["k_pad"] == 16
    # few points: the draws are split until the chip is full (two workgroups per CU)
    assert c1["splits"] > 1 and c1["splits"] * c1["point_tiles"] >= 256
    assert c1["splits"] * c1["point_tiles"] <= 2 * 2 * 256
    # point tiles alone reach the target: one split (C2 with 8 pooled chains: 157 tiles < 512,
    # still split; 40 000 points are not)
    assert plan(plan_exe, 40000, 400000, 32)["splits"] == 1
    c2 = plan(plan_exe, 10000, 50000, 32)
    assert c2["point_tiles"] == 157 and c2["splits"] == 4 and c2["k_pad"] == 32
    # a split never walks fewer than 4 draw tiles unless there are fewer draws than that
    tiny = plan(plan_exe, 1, 65, 1)
    assert tiny["splits"] == 1 and tiny["draw_tiles"] == 2
    assert plan(plan_exe, 64, 4097, 256)["k_pad"] == 256


def test_split_plan_covers_every_draw_once(plan_exe):
    """sweep: for a grid of shapes every draw tile belongs to exactly one split, no split is
    empty, and the plan passes the launcher's own consistency checks."""
    r = subprocess.run([plan_exe, "sweep"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "sweep" and int(last[1]) > 1000 and int(last[2]) == 0, r.stdout[-2000:]


# ---- argument validation (no GPU) ----------------------------------------------------------------
def test_argument_validation_needs_no_gpu():
    from pybmc_amd import scoring
    A = np.zeros((5, 3))
    y = np.zeros(5)
    th = np.ones((10, 4))
    bad = [
        (np.zeros((5, 3), dtype=np.float32), y, th, {}),          # dtype
        (A, y, th.astype(np.float32), {}),
        (A, np.zeros(4), th, {}),                                 # y length
        (A, y, np.ones((10, 5)), {}),                             # columns != k + 1
        (A, y, np.ones((1, 4)), {}),                              # S < 2
        (A, y, th, {"burn": 9}),                                  # one draw left
        (A, y, th, {"burn": -1}), (A, y, th, {"thin": 0}), (A, y, th, {"burn": 1.5}),
        (np.zeros((5, 257)), y, np.ones((10, 258)), {}),          # k > 256
        (np.zeros((0, 3)), np.zeros(0), th, {}),                  # no point
        (np.zeros(5), y, th, {}), (A, y, np.ones(4), {}),         # dimensions
        (A, y, np.ones((2, 2, 10, 4)), {}),
    ]
    for a, yy, t, kw in bad:
        with pytest.raises(ValueError):
            scoring.pointwise_log_likelihood(a, yy, t, **kw)
    assert scoring.kept_draws(10, 3, 2) == 4 and scoring.kept_draws(10, 10, 1) == 0


def test_bmc_methods_guard_call_order():
    import pandas as pd
    from pybmc_amd import BayesianModelCombination
    df = pd.DataFrame({"a": [1.0, 2.0], "b": [1.5, 2.5], "truth": [1.2, 2.2]})
    bmc = BayesianModelCombination(["a", "b"], {"p": df}, "truth")
    with pytest.raises(ValueError, match="orthogonalize"):
        bmc.waic()
    with pytest.raises(ValueError, match="orthogonalize"):
        bmc.log_predictive_density(df)


def test_new_entry_points_are_bound():
    from pybmc_amd import _lib
    import pybmc_amd
    assert "bmc_pointwise_loglik" in _lib.PROTOTYPES
    assert "bmc_pointwise_loglik_device" in _lib.PROTOTYPES
    assert callable(pybmc_amd.waic) and callable(pybmc_amd.pointwise_log_likelihood)
    lib = _lib.load_library()
    assert lib.bmc_abi_version() == 4
    # a NULL context is refused before anything touches a device
    assert lib.bmc_pointwise_loglik(None, None, 1, 1, 1, 0, None, None, 2, 2, None, None, None) == 1


def test_held_out_elpd_ranks_components_on_cpu_chains():
    """The generator of the GPU surface test, scored by the numpy reference on chains of the CPU
    oracle: three components beat one on held-out data by far more than the standard error."""
    from oracle import bmc_oracle as O
    train, models = R.three_component_frame(400, seed=1)
    val, _ = R.three_component_frame(200, seed=2)
    np.random.seed(11)
    elpd = {}
    for kept in (1, 3):
        mu, yc, U_hat, S_hat, Vt_hat, _ = O.centre_and_svd(train[models].values,
                                                           train["truth"].values, kept, False)
        prior = (np.zeros(kept), np.diag(S_hat ** 2), 1.0, 0.02)
        th = O.gibbs_port(yc, U_hat, 700, prior)[200:]
        P = val[models].values
        pw = R.pointwise(P @ Vt_hat.T, val["truth"].values - P.mean(axis=1), th)
        elpd[kept] = R.elpd_summary(pw)
    print(elpd)
    assert elpd[3]["elpd"] - elpd[1]["elpd"] > 5 * max(elpd[3]["se"], elpd[1]["se"])


@pytest.mark.parametrize("k", R.SHAPE_K)
def test_shape_cases_are_well_conditioned(k):
    """The inputs of the GPU shape test: the float64 reference is within 1e-13 of extended
    precision on every one (var_s ll of two nearly equal values would not be), so the device
    bound of 1e-11 is 100 x the reference's own error there too."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("no extended precision on this platform")
    worst = 0.0
    for case, n, S, (A, y, th) in R.shape_cases(k):
        if k == 256 and S == 4097 and n == 1000:
            A, y = A[:200], y[:200]     # (the extended-precision product is slow)
        a, b = R.pointwise(A, y, th), R.pointwise(A, y, th, dtype=np.longdouble)
        e = max(float((np.abs(a[key] - b[key]) / np.abs(b[key])).max()) for key in a)
        worst = max(worst, e)
    print(k, worst)
    assert worst < 1e-13
