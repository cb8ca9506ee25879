"""CPU checks of the leave-one-out predictive moments (pybmc_amd.scoring.psis_loo_predict,
kernels_loo.hip's PREDICT passes): the numpy reference of loo_predict_reference.py against a closed
form it did not produce, its rounding floor against np.longdouble on the cases of
test_loo_predict_gpu.py, the mirror case that tells shared ties from ties broken by index, its
invariance under permutation, the plan of bmc_plan.h (g++ builds tests/loo_predict_plan_check.cpp),
argument validation and the public surface."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import loo_predict_reference as L
import psis_reference as P
import score_reference as R
from conftest import load_golden

HERE = os.path.dirname(os.path.abspath(__file__))
EXT = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


def erfc_decimal(x, digits=120):
    """erfc(x) of a float from the alternating Taylor series of erf,
    2 / sqrt(pi) sum_n (-1)^n x^(2n+1) / (n! (2n+1)), in `digits`-digit decimal arithmetic (the
    terms reach e^(x^2) = 1.5e35 at |x| = 9: 120 digits leave 80 after the cancellation); pi from
    Machin's formula.  Standard library only, and nothing in common with the reference's series."""
    import decimal
    from decimal import Decimal as D
    with decimal.localcontext() as ctx:
        ctx.prec = digits
        eps = D(10) ** -(digits - 5)

        def atan_inv(q):        # atan(1 / q)
            t = s = D(1) / q
            n = 1
            while abs(t) > eps:
                t = -t / (q * q)
                n += 2
                s += t / n
            return s
        pi = 4 * (4 * atan_inv(D(5)) - atan_inv(D(239)))
        xd = D(float(x))        # (a float is converted exactly)
        term, s, n = xd, xd, 0  # term = (-1)^n x^(2n+1) / n!
        while abs(term) > eps:
            n += 1
            term = -term * xd * xd / n
            s += term / (2 * n + 1)
        return 1 - 2 / pi.sqrt() * s


def test_extended_erfc_against_a_decimal_series():
    """The longdouble erfc of the reference (numpy and scipy have none) at points on both sides of
    every switch of its series: within 1e-17 absolute of a 120-digit evaluation, 1 / 20 of a
    float64 eps, so that it can serve as the truth for the float64 floors (it is 1 - erf: a few eps
    of 1, more where x^2 is large and exp(-x^2) carries the rounding of its argument)."""
    from decimal import Decimal as D
    if not EXT:
        pytest.skip("no extended precision on this platform")
    assert abs(erfc_decimal(0.5) - D("0.479500122186953462317253346108035471263548")) < D("1e-40")
    xs = np.array([-7.5, -3.2, -1.1, -0.3, 0.0, 0.2, 0.74, 0.76, 1.4, 1.6, 2.4, 2.6, 3.9, 4.1, 6.5, 6.7, 9.0])
    got = L.erfc(xs.astype(np.longdouble), np.longdouble)
    for x, g in zip(xs, got):
        err = abs(D(np.format_float_scientific(g, precision=30, unique=False)) - erfc_decimal(x))
        assert err <= D("1e-17"), (x, float(err))
    z = np.linspace(-9, 9, 4001)
    assert np.abs(L.phi(z) - np.asarray(L.phi(z, np.longdouble), dtype=np.float64)).max() < 3e-16


def test_closed_form_leave_one_out_predictive():
    """closed_form_case(200, 4, 20000, 7): the exact leave-one-out predictive of point i is
    N(y_i - r_i / (1 - h_i), sigma^2 / (1 - h_i)).  Measured: |loo_mean - exact| 0.064 at row 0
    (leverage 0.5, k-hat 0.66; the plain posterior mean is 0.64 off), 1.4e-3 at most elsewhere;
    loo_sd / exact 0.963 at row 0, 0.9997 .. 1.0006 elsewhere; |loo_pit - exact| 5.3e-3 at row 0,
    5.0e-4 at most elsewhere.  The bars leave room for another seed's Monte-Carlo error."""
    A, y, th, _, _ = P.closed_form_case(200, 4, 20000, 7)
    pw = L.pointwise(A, y, th)
    mean, sd, pit = L.exact_closed_form(A, y, th)
    d_m, q_s, d_p = np.abs(pw["loo_mean"] - mean), pw["loo_sd"] / sd, np.abs(pw["loo_pit"] - pit)
    post = np.abs(A @ th[:, :-1].mean(axis=0) - mean)
    print(d_m[0], post[0], d_m[1:].max(), q_s[0], q_s[1:].min(), q_s[1:].max(), d_p[0], d_p[1:].max())
    assert d_m[1:].max() <= 5e-3
    assert 0.995 <= q_s[1:].min() and q_s[1:].max() <= 1.005
    assert d_p[1:].max() <= 2e-3
    assert d_m[0] <= 0.25 * post[0]
    assert 0.9 <= q_s[0] <= 1.1
    assert np.all((pw["ess"] >= 1) & (pw["ess"] <= 20000))
    # elpd_loo_i and pareto_k are psis_reference's: sharing ties moves neither sum
    pp = P.pointwise(A, y, th)
    for key in ("elpd_loo", "pareto_k", "lppd"):
        assert np.array_equal(pp[key], pw[key]), key


# ---- the rounding floor ---------------------------------------------------------------------------
def ties_case():
    A, y, th = R.random_case(200, 5, 9000, 77)
    rng = np.random.default_rng(3)
    rep = th[0].copy()
    rep[:5] += 0.5
    t2 = th.copy()
    t2[rng.permutation(9000)[:4500]] = rep
    return A, y, t2


def few_ulp_case():
    A, y, th = R.synth_case("c1")
    A = A.copy()
    A[5] = 0.0
    th = th.copy()[:9000]
    th[:, -1] = 0.5 * (1 + np.arange(9000) % 7 * 2.0 ** -51)
    return A, y, th


def gpu_case(name):
    if name in R.CASES:
        A, y, th = R.synth_case(name)
        return A[:400], y[:400], th     # (the extended-precision reference is slow; row 0 is the outlier)
    if name in P.GOLDEN:
        g = load_golden(name)
        return np.asarray(g["X"], dtype=np.float64), g["y"], g["samples"]
    return {"mirror": L.mirror_case, "ties": ties_case, "few_ulp": few_ulp_case}[name]()


def floors(A, y, th):
    """({key: floor of the points with k <= 1}, {key: of those with k > 1}, n with k > 1)."""
    a = L.pointwise(A, y, th)
    b = L.pointwise(A, y, th, dtype=np.longdouble)
    kb = np.asarray(b["pareto_k"], dtype=np.float64)
    assert np.array_equal(np.isinf(kb), np.isinf(a["pareto_k"]))
    big = kb > 1
    small, large = {}, {}
    for key in L.NEW_KEYS:
        d = np.asarray(np.abs(a[key] - b[key]), dtype=np.float64)
        if key == "ess":
            d = d / np.asarray(b[key], dtype=np.float64)
        small[key] = float(np.concatenate([d[~big], np.zeros(1)]).max())
        large[key] = float(np.concatenate([d[big], np.zeros(1)]).max())
    return small, large, int(big.sum())


@pytest.mark.parametrize("name", sorted(R.CASES) + list(P.GOLDEN) + ["mirror", "ties", "few_ulp"])
def test_reference_rounding_floor(name):
    """float64 reference against np.longdouble on the cases of test_loo_predict_gpu.py (the
    synthetic ones cut to their first 400 points).  Measured, loo_mean / loo_sd / loo_pit absolute
    and ess relative, points with k <= 1:
    c1 3.5e-16 / 7.8e-16 / 2.5e-16 / 5.4e-16, c2ish 5.7e-17 / 7.4e-17 / 2.6e-16 / 5.5e-16,
    tight 1.4e-17 / 1.1e-18 / 2.3e-16 / 5.7e-16, gibbs_ortho629x3 4.9e-17 / 1.5e-16 / 2.4e-16 / 5.0e-16,
    gibbs_dense64x8 5.0e-16 / 3.7e-16 / 1.6e-16 / 5.7e-15, gibbs_ragged1237x5 1.04e-15 / 2.97e-15 /
    2.9e-16 / 7.4e-16, simplex_synth150x4 2.8e-16 / 5.4e-16 / 1.5e-16 / 4.9e-16, mirror 3.4e-16 /
    2.1e-16 / 1.2e-16 / 5.68e-15, ties 3.1e-16 / 3.4e-16 / 2.5e-16 / 7.5e-16, few_ulp 4.0e-16 /
    7.7e-16 / 2.7e-16 / 5.6e-16.  Points with k > 1 (the 40-sigma outlier of c1, c2ish, tight and
    few_ulp, 93 points of ties) need a class of their own for loo_sd and ess: c1 1.49e-15 /
    6.15e-14 / 2.2e-16 / 2.1e-16, c2ish 1.1e-15 / 1.1e-14 / 2.2e-16 / 6.3e-16, few_ulp 2.2e-16 /
    2.2e-14 / 1.1e-16 / 2.09e-14, ties 2.5e-16 / 3.2e-16 / 2.1e-16 / 6.7e-16."""
    if not EXT:
        pytest.skip("no extended precision on this platform")
    small, large, n_big = floors(*gpu_case(name))
    print(name, n_big, small, large)
    for key in L.NEW_KEYS:
        assert small[key] <= L.FLOORS[key], key
        assert large[key] <= L.FLOORS_BIG[key], key


@pytest.mark.parametrize("k", (3, 33))
def test_shape_cases_are_within_the_floors(k):
    """The inputs of the GPU shape test (largest measured: loo_pit 4.18e-16 at k = 33, ess 9.6e-16)."""
    if not EXT:
        pytest.skip("no extended precision on this platform")
    worst = {key: 0.0 for key in L.NEW_KEYS}
    for case, n, S, (A, y, th) in P.shape_cases(k):
        if n == 1000 and S == 4097:
            A, y = A[:100], y[:100]         # (the extended-precision reference is slow)
        small, large, _ = floors(A, y, th)
        worst = {key: max(worst[key], small[key]) for key in worst}
        for key in L.NEW_KEYS:             # (a few points of the short cases have k > 1)
            assert large[key] <= L.FLOORS_BIG[key], (key, n, S)
    print(k, worst)
    for key in L.NEW_KEYS:
        assert worst[key] <= L.FLOORS[key], key


# ---- ties -------------------------------------------------------------------------------------------
def test_mirror_case_tells_shared_ties_from_ties_by_index():
    A, y, th = L.mirror_case()
    ll0 = R.loglik(A[:1], y[:1], th)[0]
    assert np.array_equal(ll0[:4500], ll0[4500:]) and len(np.unique(ll0)) == 4500
    r0 = y[0] - th[:, :3] @ A[0]
    assert np.array_equal(r0[:4500], -r0[4500:])
    a = L.pointwise(A[:5], y[:5], th)
    b = L.pointwise(A[:5], y[:5], th, ties="index")
    print(a["loo_mean"][0], a["loo_pit"][0] - 0.5, b["loo_mean"][0], b["loo_pit"][0] - 0.5)
    assert abs(a["loo_mean"][0]) <= 1e-12 and abs(a["loo_pit"][0] - 0.5) <= 1e-12
    assert np.isfinite(a["pareto_k"][0])        # the tail IS smoothed: the copies' ranks differ
    assert abs(b["loo_mean"][0]) > 1e-9 and abs(b["loo_pit"][0] - 0.5) > 1e-9
    for key in ("elpd_loo", "pareto_k"):
        assert np.array_equal(a[key], b[key]), key


def test_permuting_the_draws_changes_nothing():
    rng = np.random.default_rng(0)
    g = load_golden("simplex_synth150x4")          # rejected proposals repeat the coefficients
    for A, y, th in ((np.asarray(g["X"], dtype=np.float64), g["y"], g["samples"]),
                     L.mirror_case(), tuple(v[:60] if i < 2 else v for i, v in enumerate(ties_case()))):
        base = L.pointwise(A, y, th)
        perm = L.pointwise(A, y, th[rng.permutation(len(th))])
        for key in ("loo_mean", "loo_sd", "loo_pit"):
            np.testing.assert_allclose(perm[key], base[key], rtol=0, atol=1e-12, err_msg=key)
        np.testing.assert_allclose(perm["ess"], base["ess"], rtol=1e-12, atol=0)


def test_summary_is_the_reference_summary():
    from pybmc_amd import scoring
    g = load_golden("gibbs_ortho629x3")
    A, y, th = np.asarray(g["X"], dtype=np.float64), g["y"], g["samples"]
    pw = L.pointwise(A, y, th)
    mine = scoring.loo_predict_summary(y, pw["loo_mean"], pw["loo_pit"], pw["ess"])
    ref = L.summary(y, pw)
    assert set(mine) == set(ref) == {"loo_rmse", "pit_coverage", "min_ess"}
    assert mine["loo_rmse"] == pytest.approx(ref["loo_rmse"], rel=1e-12)
    assert mine["min_ess"] == ref["min_ess"] and 1 <= mine["min_ess"] <= len(th)
    cov = mine["pit_coverage"]
    assert cov == pytest.approx(ref["pit_coverage"]) and len(cov) == 21
    assert cov[0] == 0 and cov[-1] == 100 and np.all(np.diff(cov) >= 0)
    # a well-specified fit is calibrated: the central 50 % interval holds about half the points
    assert abs(cov[10] - 50) < 8
    in_sample = np.sqrt(np.mean((y - A @ th[:, :-1].mean(axis=0)) ** 2))
    assert in_sample <= mine["loo_rmse"] <= 1.05 * in_sample
    # a pit outside [0, 1] (NaN: a point with non-finite input) is covered at no level
    s = scoring.loo_predict_summary(np.zeros(2), np.zeros(2), np.array([0.5, np.nan]), np.ones(2))
    assert s["pit_coverage"][0] == 50 and s["pit_coverage"][-1] == 50


# ---- the plan ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is required")
    exe = tmp_path_factory.mktemp("loo_predict_plan") / "loo_predict_plan_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                        os.path.join(HERE, "loo_predict_plan_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def plan(exe, n, S, k, n_cu=256):
    r = subprocess.run([exe, "plan", str(n), str(S), str(k), str(n_cu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return dict((kv.split("=")[0], int(kv.split("=")[1])) for kv in r.stdout.split())


def test_plan_named_shapes(plan_exe):
    c1 = plan(plan_exe, 377, 50000, 3)
    c2 = plan(plan_exe, 10000, 50000, 32)
    for p in (c1, c2):
        assert p["tail"] == 671 and p["cap"] == 2048 and p["fit_lds"] == 32768 and p["ok"] == 1
        assert p["bucket_pass"] == 1 and p["matrix_passes"] == 12 and p["record_bytes"] == 12
    assert c2["workspace"] < 10000 * (12 * 2048 + 256 * 4 + 4 * 100) * 1.1     # O(n (cap + splits))
    small = plan(plan_exe, 629, 64, 3)
    assert small["select_passes"] == 0 and small["bucket_pass"] == 0 and small["matrix_passes"] == 3
    assert plan(plan_exe, 10, 24, 3)["tail"] == 0 and plan(plan_exe, 10, 24, 3)["bucket_pass"] == 0
    # the draw limit: 16 bytes of LDS per slot, cap 8192, M <= 4095
    top = plan(plan_exe, 100, 1863225, 3)
    assert top["ok"] == 1 and top["tail"] == 4095 and top["cap"] == 8192 and top["fit_lds"] == 131072
    assert top["max_draws"] == 1863225 == 4095 ** 2 // 9
    over = plan(plan_exe, 100, 1863226, 3)
    assert over["ok"] == 0 and over["tail"] == 4096


def test_plan_sweep(plan_exe):
    r = subprocess.run([plan_exe, "sweep"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "sweep" and int(last[1]) > 70000 and int(last[2]) == 0, r.stdout[-2000:]


# ---- argument validation and the surface (no GPU) ---------------------------------------------------
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
            scoring.psis_loo_predict(a, yy, t, **kw)
        with pytest.raises(ValueError) as e2:
            scoring.psis_loo(a, yy, t, **kw)
        assert str(e1.value) == str(e2.value)


def test_bmc_loo_predict_guards_call_order():
    import pandas as pd
    from pybmc_amd import BayesianModelCombination
    df = pd.DataFrame({"a": [1.0, 2.0], "b": [1.5, 2.5], "truth": [1.2, 2.2]})
    bmc = BayesianModelCombination(["a", "b"], {"p": df}, "truth")
    with pytest.raises(ValueError, match="orthogonalize"):
        bmc.loo_predict()
    bmc.orthogonalize("p", df, components_kept=1)
    with pytest.raises(ValueError, match="train"):
        bmc.loo_predict()


def test_new_entry_points_are_bound():
    from pybmc_amd import _lib
    import pybmc_amd
    names = ("bmc_psis_loo_predict", "bmc_psis_loo_predict_device")
    header = open(os.path.join(HERE, "..", "include", "pybmc_amd.h")).read()
    for name in names:
        assert name in _lib.PROTOTYPES and name + "(" in header
        assert len(_lib.PROTOTYPES[name][1]) == len(_lib.PROTOTYPES["bmc_psis_loo"][1]) + 4
    assert callable(pybmc_amd.psis_loo_predict) and "psis_loo_predict" in pybmc_amd.__all__
    assert callable(pybmc_amd.scoring.loo_predict_summary)
    assert callable(pybmc_amd.BayesianModelCombination.loo_predict)
    assert callable(_lib.Context.psis_loo_predict) and callable(_lib.Context.psis_loo_predict_device)
    lib = _lib.load_library()
    assert lib.bmc_abi_version() == 4
    # a NULL context is refused before anything touches a device
    null = (None, None, 1, 1, 1, 0, None, None, 2, 2) + (None,) * 7
    assert lib.bmc_psis_loo_predict(*null) == 1
    assert lib.bmc_psis_loo_predict_device(*null) == 1
