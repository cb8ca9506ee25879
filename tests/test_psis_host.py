"""CPU checks of the PSIS-LOO feature (pybmc_amd.scoring.psis_loo, kernels_loo.hip's plan): the
numpy reference of psis_reference.py against things it did not produce (exact generalised Pareto
quantiles, a closed-form leave-one-out density), its rounding floor against np.longdouble on the
cases of test_psis_gpu.py, its invariance under ties, the plan of bmc_plan.h (g++ builds
tests/loo_plan_check.cpp), argument validation."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import psis_reference as P
import score_reference as R
from conftest import load_golden

HERE = os.path.dirname(os.path.abspath(__file__))
EXT = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps

# the floors test_psis_gpu.py derives its bars from (100 x): measured by
# test_reference_rounding_floor below, rounded up in the second digit
FLOOR_ELPD, FLOOR_K, FLOOR_ELPD_BIG = 3.1e-15, 1.2e-12, 6.9e-16


def test_gpdfit_on_exact_quantiles():
    """Zhang & Stephens' estimator on the exact quantiles x_j = sigma0 expm1(-k0 log1p(-p_j)) / k0,
    M = 671, sigma0 = 2: it is close to, not exact on, quantiles.  Measured, prior undone
    (float64 and longdouble agree to 2e-14): k = -0.29524, 0.10257, 0.50061, 0.89850 for
    k0 = -0.3, 0.1, 0.5, 0.9 (largest |k - k0| 4.8e-3), sigma = 1.98992, 1.99374, 1.99724, 2.00104
    (largest relative error 0.51 %).  Bars: 5e-3 and 0.6 %."""
    M, sigma0 = 671, 2.0
    for k0 in (-0.3, 0.1, 0.5, 0.9):
        res = []
        for dt in (np.float64, np.longdouble):
            p = (np.arange(1, M + 1).astype(dt) - dt(0.5)) / M
            x = dt(sigma0) * np.expm1(-dt(k0) * np.log1p(-p)) / dt(k0)
            k, s = P.gpdfit(x, dt)
            res.append((float(P.undo_prior(k, M)), float(s)))
        (k64, s64), (kld, sld) = res
        print(k0, k64, s64, abs(k64 - kld), abs(s64 - sld))
        assert abs(k64 - kld) < 1e-12 and abs(s64 - sld) < 1e-12
        assert abs(k64 - k0) <= 5e-3 and abs(s64 / sigma0 - 1) <= 6e-3


def test_closed_form_leave_one_out_and_waic_at_a_high_leverage_point():
    """Orthonormal A (200 x 4, row 0 with h_0 = 0.50 .. 0.55), sigma = 0.7 fixed, 4000 draws
    beta_s ~ N(A'y, sigma^2 I): sum_i elpd_loo_i of the reference against the exact leave-one-out
    density.  Measured over seeds 0 .. 19: largest |deviation| 0.0931 (sd 0.049; the sum is about
    -218), so the bar is 4 x 0.0931 = 0.373.  At the high-leverage point the mean |error| of WAIC
    over the seeds (0.071) is larger than PSIS-LOO's (0.030): the reason for the feature."""
    dev, e_loo, e_waic, k0 = [], [], [], []
    for seed in range(20):
        A, y, th, exact, _ = P.closed_form_case(200, 4, 4000, seed)
        assert abs(np.sum(A[0] ** 2) - 0.5) < 0.05   # (the other three columns add O(k / n))
        pw = P.pointwise(A, y, th)
        sw = R.pointwise(A, y, th)
        dev.append(float(pw["elpd_loo"].sum() - exact.sum()))
        e_loo.append(abs(float(pw["elpd_loo"][0] - exact[0])))
        e_waic.append(abs(float(sw["lppd"][0] - sw["p_waic"][0] - exact[0])))
        k0.append(float(pw["pareto_k"][0]))
    print(np.abs(dev).max(), np.std(dev), np.mean(e_loo), np.mean(e_waic), np.mean(k0))
    assert np.abs(dev).max() <= 0.373
    assert np.mean(e_waic) > np.mean(e_loo)
    assert 0.3 < np.mean(k0) < 0.7          # k-hat of a Gaussian ratio with h = 0.5 is about h


def gpu_cases():
    for name in sorted(R.CASES):
        yield name, R.synth_case(name)
    for name in P.GOLDEN:
        g = load_golden(name)
        yield name, (np.asarray(g["X"], dtype=np.float64), g["y"], g["samples"])


def floors(A, y, th):
    """(elpd floor of ordinary points, of points with k > 1, k floor of ordinary points, n big)."""
    a = P.pointwise(A, y, th)
    b = P.pointwise(A, y, th, dtype=np.longdouble)
    kb = np.asarray(b["pareto_k"], dtype=np.float64)
    assert np.array_equal(np.isinf(kb), np.isinf(a["pareto_k"]))
    big = kb > 1
    fe = np.asarray(np.abs(a["elpd_loo"] - b["elpd_loo"]) / np.maximum(1, np.abs(b["elpd_loo"])),
                    dtype=np.float64)
    fk = np.where(np.isinf(kb), 0.0, np.abs(np.where(np.isinf(kb), 0.0, a["pareto_k"] - kb)))
    z = np.zeros(1)
    return (np.concatenate([fe[~big], z]).max(), np.concatenate([fe[big], z]).max(),
            np.concatenate([fk[~big], z]).max(), int(big.sum()))


@pytest.mark.parametrize("name", sorted(R.CASES) + list(P.GOLDEN))
def test_reference_rounding_floor(name):
    """float64 reference against np.longdouble on the cases of test_psis_gpu.py; no point left out.
    Measured (elpd_loo_i relative to max(1, |ref|) / pareto_k absolute, points with k <= 1):
    c1 3.04e-15 / 1.54e-14, c2ish 2.52e-15 / 4.71e-14, tight 1.90e-15 / 1.18e-12,
    gibbs_ortho629x3 1.66e-15 / 8.50e-14, gibbs_dense64x8 1.34e-15 / 1.81e-14,
    gibbs_ragged1237x5 1.33e-15 / 2.45e-14, simplex_synth150x4 1.48e-15 / 1.43e-14.  The one point
    with k > 1 of each synthetic case (the 40-sigma outlier, k-hat 19.9 / 9.75 / 9.47): elpd_loo_0
    6.89e-16 / 1.31e-16 / 2.25e-16.  No float64 reference is unstable (all far below 1e-9)."""
    if not EXT:
        pytest.skip("no extended precision on this platform")
    cases = dict(gpu_cases())
    fe, fe_big, fk, n_big = floors(*cases[name])
    print(name, fe, fe_big, fk, n_big)
    assert n_big == (1 if name in R.CASES else 0)
    assert fe <= FLOOR_ELPD and fe_big <= FLOOR_ELPD_BIG and fk <= FLOOR_K
    assert max(fe, fe_big, fk) < 1e-9


def test_reference_on_the_named_cases():
    """What the estimator says about the repository's own cases: the outlier of synth_case is the
    one point with a high k-hat, the reference's own chains have none."""
    for name, want_k, want_e in (("c1", 19.9, -1051.0), ("c2ish", 9.75, -913.0), ("tight", 9.47, -890.0)):
        A, y, th = R.synth_case(name)
        pw = P.pointwise(A[:40], y[:40], th)
        assert pw["pareto_k"][0] == pytest.approx(want_k, abs=0.06)
        assert pw["elpd_loo"][0] == pytest.approx(want_e, abs=0.6)
        assert np.all(np.abs(pw["pareto_k"][1:]) < 0.3)
    g = load_golden("gibbs_ortho629x3")
    A, y, th = np.asarray(g["X"], dtype=np.float64), g["y"], g["samples"]
    pw = P.pointwise(A, y, th)
    s = P.loo_summary(pw, len(th))
    assert P.tail_length(len(th)) == 135 and pw["pareto_k"].max() <= 0.23 and s["n_high_k"] == 0
    # p_loo is close to p_waic (4.243) and elpd_loo to elpd_waic (522.75) on a well-behaved fit
    assert s["p_loo"] == pytest.approx(4.25, abs=0.05) and s["elpd_loo"] == pytest.approx(522.75, abs=0.05)
    assert s["looic"] == -2.0 * s["elpd_loo"] and s["k_threshold"] == pytest.approx(1 - 1 / np.log10(2000))
    from pybmc_amd import scoring
    mine = scoring.loo_summary(pw["elpd_loo"], pw["lppd"], pw["pareto_k"], len(th))
    assert set(mine) == set(s)
    for key, v in s.items():
        assert mine[key] == pytest.approx(v, rel=1e-9), key


def test_ties_are_by_value():
    """The simplex sampler's chains repeat the coefficients on every rejection (sigma is drawn anew),
    and duplicated draws tie exactly.  Permuting the draws changes
    nothing beyond rounding; duplicating every draw (S -> 2S changes M) equals the reference on the
    duplicated input in any order."""
    g = load_golden("simplex_synth150x4")
    A, y, th = np.asarray(g["X"], dtype=np.float64), g["y"], g["samples"]
    assert len(np.unique(th[:, :-1], axis=0)) < len(th)    # rejected proposals repeat the coefficients
    rng = np.random.default_rng(0)
    base = P.pointwise(A, y, th)
    perm = P.pointwise(A, y, th[rng.permutation(len(th))])
    np.testing.assert_allclose(perm["elpd_loo"], base["elpd_loo"], rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(perm["pareto_k"], base["pareto_k"], rtol=0, atol=1e-11)
    dup = np.repeat(th, 2, axis=0)
    a = P.pointwise(A, y, dup)
    b = P.pointwise(A, y, dup[rng.permutation(len(dup))])
    assert P.tail_length(len(dup)) != P.tail_length(len(th))
    np.testing.assert_allclose(b["elpd_loo"], a["elpd_loo"], rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(b["pareto_k"], a["pareto_k"], rtol=0, atol=1e-11)
    # a tail of equal values is not smoothed; fewer than 25 draws neither
    e, k = P.psis_row(np.full(100, -1.25))
    assert np.isinf(k) and e == pytest.approx(-1.25, abs=1e-14)
    e, k = P.psis_row(np.linspace(-2, -1, 24))
    assert np.isinf(k)
    assert np.isfinite(P.psis_row(np.linspace(-2, -1, 25))[1])


@pytest.mark.parametrize("k", R.SHAPE_K)
def test_shape_cases_are_well_conditioned(k):
    """The inputs of the GPU shape test: the float64 reference is within the floors of the named
    cases on every one, so the device bars are 100 x the reference's own error there too."""
    if not EXT:
        pytest.skip("no extended precision on this platform")
    worst = np.zeros(3)
    for case, n, S, (A, y, th) in P.shape_cases(k):
        if n == 1000 and (S == 4097 or k == 256):
            A, y = A[:100], y[:100]         # (the extended-precision reference is slow)
        worst = np.maximum(worst, floors(A, y, th)[:3])
    print(k, worst)
    assert worst[0] <= FLOOR_ELPD and worst[1] <= FLOOR_ELPD_BIG and worst[2] <= FLOOR_K


# ---- the plan ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is required")
    exe = tmp_path_factory.mktemp("loo_plan") / "loo_plan_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                        os.path.join(HERE, "loo_plan_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def plan(exe, n, S, k, n_cu=256):
    r = subprocess.run([exe, "plan", str(n), str(S), str(k), str(n_cu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return dict((kv.split("=")[0], int(kv.split("=")[1])) for kv in r.stdout.split())


def test_plan_named_shapes(plan_exe):
    for S in (25, 400, 2000, 50000, 400000):
        assert plan(plan_exe, 377, S, 3)["tail"] == P.tail_length(S)
    c2 = plan(plan_exe, 10000, 50000, 32)
    assert c2["tail"] == 671 and c2["cap"] == 2048 and c2["splits"] == 4 and c2["matrix_passes"] == 11
    big = plan(plan_exe, 10000, 400000, 32)
    assert big["tail"] == 1898 and big["cap"] == 4096
    assert big["workspace"] < 10000 * (1898 + 256 + 4 * 8) * 8 * 3     # O(n (M + splits))
    assert plan(plan_exe, 10, 24, 3)["tail"] == 0 and plan(plan_exe, 10, 24, 3)["select_passes"] == 0
    assert plan(plan_exe, 629, 64, 3)["select_passes"] == 0            # every draw is a candidate
    assert plan(plan_exe, 629, 2000, 3)["cap"] == 512
    assert plan(plan_exe, 100, 7454720, 3)["ok"] == 1 and plan(plan_exe, 100, 7454721, 3)["ok"] == 0


def test_plan_sweep(plan_exe):
    r = subprocess.run([plan_exe, "sweep"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "sweep" and int(last[1]) > 70000 and int(last[2]) == 0, r.stdout[-2000:]


# ---- argument validation (no GPU) -------------------------------------------------------------------
def test_argument_validation_needs_no_gpu():
    from pybmc_amd import scoring
    A = np.zeros((5, 3))
    y = np.zeros(5)
    th = np.ones((10, 4))
    bad = [
        (np.zeros((5, 3), dtype=np.float32), y, th, {}), (A, y, th.astype(np.float32), {}),
        (A, np.zeros(4), th, {}), (A, y, np.ones((10, 5)), {}), (A, y, np.ones((1, 4)), {}),
        (A, y, th, {"burn": 9}), (A, y, th, {"burn": -1}), (A, y, th, {"thin": 0}),
        (A, y, th, {"burn": 1.5}), (np.zeros((5, 257)), y, np.ones((10, 258)), {}),
        (np.zeros((0, 3)), np.zeros(0), th, {}), (np.zeros(5), y, th, {}), (A, y, np.ones(4), {}),
        (A, y, np.ones((2, 2, 10, 4)), {}),
    ]
    for a, yy, t, kw in bad:
        with pytest.raises(ValueError) as e1:
            scoring.psis_loo(a, yy, t, **kw)
        with pytest.raises(ValueError) as e2:
            scoring.pointwise_log_likelihood(a, yy, t, **kw)
        assert str(e1.value) == str(e2.value)


def test_bmc_loo_guards_call_order():
    import pandas as pd
    from pybmc_amd import BayesianModelCombination
    df = pd.DataFrame({"a": [1.0, 2.0], "b": [1.5, 2.5], "truth": [1.2, 2.2]})
    bmc = BayesianModelCombination(["a", "b"], {"p": df}, "truth")
    with pytest.raises(ValueError, match="orthogonalize"):
        bmc.loo()


def test_new_entry_points_are_bound():
    from pybmc_amd import _lib
    import pybmc_amd
    assert "bmc_psis_loo" in _lib.PROTOTYPES and "bmc_psis_loo_device" in _lib.PROTOTYPES
    assert callable(pybmc_amd.psis_loo) and "psis_loo" in pybmc_amd.__all__
    assert callable(pybmc_amd.scoring.loo_summary)
    lib = _lib.load_library()
    assert lib.bmc_abi_version() == 4
    # a NULL context is refused before anything touches a device
    assert lib.bmc_psis_loo(None, None, 1, 1, 1, 0, None, None, 2, 2, None, None, None) == 1
    assert lib.bmc_psis_loo_device(None, None, 1, 1, 1, 0, None, None, 2, 2, None, None, None) == 1
