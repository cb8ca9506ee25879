"""CPU checks of the leave-one-out predictive moments under the Student-t likelihood
(pybmc_amd.scoring.psis_loo_predict(nu= / nu_draws=), BayesianModelCombination.loo_predictions,
kernels_loo.hip's t PREDICT passes): bmc_math.h's student_t_cdf (g++ build) against mpmath, closed
forms and its own symmetry; the numpy reference of loo_predict_t_reference.py, its long-double
distribution function against mpmath and its rounding floor on the cases of
test_loo_predict_t_gpu.py; the plan's new fields (g++ builds tests/loo_predict_t_plan_check.cpp);
the Python surface with a fake context; the C ABI's refusals."""
import os
import shutil
import subprocess
import threading

import numpy as np
import pytest

import loo_predict_t_host_build as HB
import loo_predict_t_reference as LT
import psis_reference as P
import tscore_reference as T

HERE = os.path.dirname(os.path.abspath(__file__))
EXT = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


def cdf_grid(nu, n_variates=300):
    """The arguments of the distribution-function checks at one nu: t variates (seeded) and the
    special values in both signs, with the infinities and a NaN last."""
    rng = np.random.default_rng(int(round(nu * 100)) + 5)
    z = rng.standard_t(nu, n_variates)
    z = z[np.abs(z) < 1e150]           # (z^2 must be a double: bmc_math.h)
    sp = np.array(LT.CDF_SPECIAL)
    return np.concatenate([z, sp, -sp, [np.inf, -np.inf, np.nan]])


def mp_cdf(z, nu):
    """F_nu(z) of finite z at 40 digits, as mpmath numbers."""
    import mpmath as mp
    out = []
    with mp.workdps(40):
        for v in z:
            zz, n = mp.mpf(float(v)), mp.mpf(float(nu))
            tail = mp.betainc(n / 2, mp.mpf(1) / 2, 0, n / (n + zz * zz), regularized=True) / 2
            out.append(tail if v < 0 else 1 - tail)
    return out


def abs_err(got, want):
    import mpmath as mp
    with mp.workdps(40):
        return max(float(abs(mp.mpf(float(g)) - w)) for g, w in zip(got, want))


# ---- student_t_cdf of bmc_math.h ----------------------------------------------------------------------
@pytest.mark.parametrize("nu", LT.CDF_NUS)
def test_student_t_cdf_against_mpmath(nu):
    """The g++ build of student_t_cdf on a few hundred t variates and the special arguments: the
    largest absolute error is at most 64 x that of scipy.special.stdtr on the same arguments
    (DESIGN.md 4.9's margin for device math that is not correctly rounded).  Measured, ours / stdtr:
    nu 0.06 6.2e-16 / 1.8e-16, 0.3 2.5e-16 / 2.4e-16, 1 2.9e-16 / 2.5e-16, 1.5 3.0e-16 / 2.9e-16,
    2 1.3e-16 / 1.4e-16, 2.5 2.7e-16 / 3.4e-16, 4 1.6e-16 / 2.8e-16, 17.3 2.9e-16 / 1.6e-16,
    50 2.5e-16 / 2.3e-16, 100 3.6e-16 / 2.4e-16, 1000 1.8e-15 / 2.1e-16 (8.5 times stdtr's, the
    largest ratio); at most 48 steps of the 80 allowed."""
    from scipy.special import stdtr
    z = cdf_grid(nu)
    F, steps, f = HB.t_cdf(z, nu)
    assert np.isnan(F[-1]) and F[-3] == 1.0 and F[-2] == 0.0          # NaN, +inf, -inf
    zf, Ff = z[:-3], F[:-3]
    assert np.all((Ff >= 0) & (Ff <= 1))
    want = mp_cdf(zf, nu)
    err = abs_err(Ff, want)
    floor = abs_err(stdtr(nu, zf), want)
    nu_min, nu_max, cap = HB.limits()
    print(f"nu={nu}: student_t_cdf {err:.3e}  stdtr {floor:.3e}  ratio {err / floor:.1f}  "
          f"steps <= {int(steps.max())} of {cap}")
    assert err <= 64 * floor
    assert steps.max() < cap                                          # the cap is not reached
    assert (nu_min, nu_max) == LT.NU_RANGE
    # F(0) = 1/2 exactly, the two sides mirror, and F does not decrease
    assert HB.t_cdf(np.array([0.0, -0.0]), nu)[0].tolist() == [0.5, 0.5]
    Fm = HB.t_cdf(-zf, nu)[0]
    assert np.abs(Ff + Fm - 1).max() <= 2.0 ** -52
    grid = np.sort(np.concatenate([zf, np.linspace(-6, 6, 401)]))
    Fg = HB.t_cdf(grid, nu)[0]
    assert np.all(np.diff(Fg) >= 0), np.diff(Fg).min()


def test_student_t_cdf_closed_forms():
    """Independent pins: F_1(z) = 1/2 + atan(z) / pi and F_2(z) = 1/2 + z / (2 sqrt(2 + z^2)),
    evaluated by mpmath at 40 digits, within 64 float64 eps / 2 (absolute; measured 2.9e-16 and 1.3e-16)."""
    import mpmath as mp
    for nu, form in ((1.0, lambda z: mp.mpf(1) / 2 + mp.atan(z) / mp.pi),
                     (2.0, lambda z: mp.mpf(1) / 2 + z / (2 * mp.sqrt(2 + z * z)))):
        z = cdf_grid(nu)[:-3]
        F = HB.t_cdf(z, nu)[0]
        with mp.workdps(40):
            err = abs_err(F, [form(mp.mpf(float(v))) for v in z])
        print(nu, err)
        assert err <= 64 * 2.0 ** -53


def test_steps_stay_below_the_cap_over_the_domain():
    """A scan of nu over the whole domain, |z| from 1e-3 to 1e6 and densely around the switch between
    the two branches (u = 3 / (nu + 2)), where the fraction is slowest: 55 steps at most (at nu = 372)."""
    nu_min, nu_max, cap = HB.limits()
    nus = np.geomspace(nu_min, nu_max, 80)
    worst = 0
    for nu in nus:
        sw = np.sqrt(3 * nu / (nu + 2))
        z = np.concatenate([sw * np.geomspace(0.5, 2, 81), np.geomspace(1e-3, 1e6, 91)])
        F, steps, _ = HB.t_cdf(z, nu)
        worst = max(worst, int(steps.max()))
        assert np.all(np.diff(F[np.argsort(z)]) >= 0)
    print("most steps:", worst)
    assert worst < cap


# ---- the reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu", LT.CDF_NUS)
def test_long_double_cdf_of_the_reference_against_mpmath(nu):
    """The reference's own continued fraction in np.longdouble: within 1e-17 of mpmath (1 / 20 of a
    float64 eps: it can serve as the truth for the float64 floors).  Measured: 3.6e-18 at nu = 0.06,
    below 1e-18 for nu = 1 .. 17.3, 9.4e-18 at nu = 1000 (the density's exponent carries the rounding
    of its argument)."""
    if not EXT:
        pytest.skip("no extended precision on this platform")
    z = cdf_grid(nu)
    got = LT.t_cdf(z, nu, np.longdouble)
    assert np.isnan(got[-1]) and got[-3] == 1 and got[-2] == 0
    import mpmath as mp
    with mp.workdps(40):
        err = max(float(abs(mp.mpf(np.format_float_scientific(g, precision=30, unique=False)) - w))
                  for g, w in zip(got[:-3], mp_cdf(z[:-3], nu)))
    print(nu, err)
    assert err <= 1e-17
    assert np.abs(LT.t_cdf(z[:-3], nu) - np.asarray(got[:-3], dtype=np.float64)).max() < 5e-16


def test_the_variance_rule_and_the_gaussian_limit():
    """nu <= 2 anywhere: loo_sd is +inf at every point and nothing else changes; a very large nu is
    the Gaussian estimator of loo_predict_reference.py to 1e-3 of the predictive sd."""
    import loo_predict_reference as L
    A, y, th = T.shape_case(4, 63, 130)
    a = LT.pointwise(A, y, th, nu_draws=LT.cycling(130, LT.CYCLE_INF))
    assert np.isinf(a["loo_sd"]).all() and np.isfinite(a["loo_pit"]).all()
    b = LT.pointwise(A, y, th, nu=2.0)
    assert np.isinf(b["loo_sd"]).all()
    c = LT.pointwise(A, y, th, nu_draws=LT.cycling(130, LT.CYCLE_FINITE))
    assert np.isfinite(c["loo_sd"]).all() and np.all(c["loo_sd"] > 0)
    g = L.pointwise(A, y, th)
    t = LT.pointwise(A, y, th, nu=1000.0)
    np.testing.assert_allclose(t["loo_pit"], g["loo_pit"], atol=2e-3)
    np.testing.assert_allclose(t["loo_sd"], g["loo_sd"], rtol=5e-3)
    # elpd_loo_i, pareto_k and lppd are tscore_reference's: the same weights
    lp = T.loo_pointwise(A, y, th, 4.0)
    pw = LT.pointwise(A, y, th, nu=4.0)
    for key in ("elpd_loo", "pareto_k", "lppd"):
        assert np.array_equal(lp[key], pw[key]), key
    A2 = A.copy()
    A2[7, 1] = np.nan
    bad = LT.pointwise(A2, y, th, nu=2.0)
    assert all(np.isnan(bad[key][7]) for key in LT.NEW_KEYS) and np.isinf(bad["loo_sd"][8])


def test_mirror_case_under_the_t_likelihood():
    import loo_predict_reference as L
    A, y, th = L.mirror_case()
    for lik in ({"nu": 4.0}, {"nu_draws": LT.cycling(len(th), LT.CYCLE_FINITE)}):
        ll0 = LT.loglik(A[:1], y[:1], th, **lik)[0]
        assert np.array_equal(ll0[:4500], ll0[4500:])
        a = LT.pointwise(A[:3], y[:3], th, **lik)
        print(a["loo_mean"][0], a["loo_pit"][0] - 0.5)
        assert abs(a["loo_mean"][0]) <= 1e-12 and abs(a["loo_pit"][0] - 0.5) <= 1e-12


def floors(A, y, th, lik):
    """({key: floor of the points with k <= 1}, {key: of those with k > 1}, n with k > 1)."""
    a = LT.pointwise(A, y, th, **lik)
    b = LT.pointwise(A, y, th, dtype=np.longdouble, **lik)
    kb = np.asarray(b["pareto_k"], dtype=np.float64)
    assert np.array_equal(np.isinf(kb), np.isinf(a["pareto_k"]))
    big = kb > 1
    small, large = {}, {}
    for key in LT.NEW_KEYS:
        fin = np.isfinite(np.asarray(b[key], dtype=np.float64))
        assert np.array_equal(fin, np.isfinite(a[key])), key
        with np.errstate(invalid="ignore"):        # (inf - inf where loo_sd is +inf in both)
            d = np.where(fin, np.asarray(np.abs(a[key] - b[key]), dtype=np.float64), 0.0)
        if key == "ess":
            d = d / np.asarray(b[key], dtype=np.float64)
        small[key] = float(np.concatenate([d[~big], np.zeros(1)]).max())
        large[key] = float(np.concatenate([d[big], np.zeros(1)]).max())
    return small, large, int(big.sum())


def test_reference_rounding_floor():
    """float64 reference against np.longdouble on every case of test_loo_predict_t_gpu.py (cases of
    more than 600 draws cut to their first 8 points, the others to their first 32: the
    extended-precision reference is slow; the planted outlier, which sets the floors, is point 0).
    Measured over all of them, loo_mean / loo_sd / loo_pit absolute and ess relative: points with
    k <= 1 9.31e-15 / 1.65e-13 / 3.15e-16 / 1.12e-15 (the first 100 points of every case, a run of
    2.4 minutes: 9.31e-15 / 1.65e-13 / 4.56e-16 / 1.66e-15, which are the floors recorded); points
    with k > 1 7.87e-15 / 4.53e-13 / 3.33e-16 / 3.73e-15 (the same with 100 points)."""
    if not EXT:
        pytest.skip("no extended precision on this platform")
    worst, worst_big = ({key: 0.0 for key in LT.NEW_KEYS} for _ in range(2))
    for tag, (A, y, th), spec in LT.all_cases():
        cut = 32 if len(th) <= 600 else 8
        small, large, n_big = floors(A[:cut], y[:cut], th, LT.lik_of(spec, len(th)))
        for key in LT.NEW_KEYS:
            if small[key] > worst[key] or large[key] > worst_big[key]:
                print(tag, key, small[key], large[key], n_big)
            worst[key] = max(worst[key], small[key])
            worst_big[key] = max(worst_big[key], large[key])
    print(worst, worst_big)
    for key in LT.NEW_KEYS:
        assert worst[key] <= LT.FLOORS[key], key
        assert worst_big[key] <= LT.FLOORS_BIG[key], key


# ---- the plan -------------------------------------------------------------------------------------------
def test_plan_fields_of_the_t_passes(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is required")
    exe = tmp_path / "loo_predict_t_plan_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                        os.path.join(HERE, "loo_predict_t_plan_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), "sweep"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "sweep" and int(last[1]) > 4000 and int(last[2]) == 0, r.stdout[-2000:]
    r = subprocess.run([str(exe), "plan", "10000", "50000", "32", "256"], capture_output=True, text=True)
    p = dict((kv.split("=")[0], int(kv.split("=")[1])) for kv in r.stdout.split())
    assert p["append_phases"] == 2 and p["draw_rows"] == 100000 and p["matrix_passes"] == 13
    assert p["gaussian_matrix_passes"] == 12 and p["tc_bytes"] == 800000 and p["ok"] == 1


# ---- the Python surface (no GPU) ------------------------------------------------------------------------
class FakeCtx:
    lock = threading.RLock()

    def __init__(self, calls):
        self.calls = calls

    def __getattr__(self, name):
        def call(*a):
            self.calls.append((name, a[9:]))
            n = a[1]
            return {key: np.full(n, 0.5) for key in ("elpd_loo", "pareto_k", "lppd", "loo_mean", "loo_sd",
                                                     "loo_pit", "ess")}
        return call


def test_nu_routes_to_the_t_entry_points(monkeypatch):
    import pybmc_amd
    from pybmc_amd import _lib
    calls = []
    monkeypatch.setattr(_lib, "default_context", lambda device=0: FakeCtx(calls))
    A, y, th = T.shape_case(4, 63, 25)
    pybmc_amd.psis_loo_predict(A, y, th)
    pybmc_amd.psis_loo_predict(A, y, th, nu=None, nu_draws=None)
    pybmc_amd.psis_loo_predict(A, y, th, nu=4)
    out = pybmc_amd.psis_loo_predict(A, y, th, nu_draws=LT.cycling(25, LT.CYCLE_INF))
    assert [c[0] for c in calls] == ["psis_loo_predict", "psis_loo_predict", "psis_loo_predict_t",
                                     "psis_loo_predict_tv"]
    assert calls[0][1] == () and calls[2][1] == (4.0,)
    values, index = calls[3][1]
    assert values.tolist() == [1.5, 4.0, 50.0] and index.dtype == np.int32
    assert index.tolist() == [s % 3 for s in range(25)]
    assert {"loo_mean", "loo_sd", "loo_pit", "ess", "loo_rmse", "pit_coverage", "elpd_loo"} <= set(out)


def test_bad_likelihood_arguments_raise_before_any_device_work(monkeypatch):
    import pybmc_amd
    from pybmc_amd import _lib

    def no_device(*a, **kw):
        raise AssertionError("argument errors must be raised before any device work")

    monkeypatch.setattr(_lib, "default_context", no_device)
    A, y, th = T.shape_case(4, 63, 25)
    with pytest.raises(ValueError, match="not both"):
        pybmc_amd.psis_loo_predict(A, y, th, nu=4.0, nu_draws=np.full(25, 4.0))
    for nu in (0.05, 1000.5, 1e6):
        with pytest.raises(ValueError, match="between 0.06 and 1000"):
            pybmc_amd.psis_loo_predict(A, y, th, nu=nu)
    for nu in (0, -1.0, float("nan"), float("inf"), "4", True):
        with pytest.raises(ValueError, match="nu must be"):
            pybmc_amd.psis_loo_predict(A, y, th, nu=nu)
    nd = np.full(25, 4.0)
    nd[7] = 0.01
    with pytest.raises(ValueError, match="between 0.06 and 1000"):
        pybmc_amd.psis_loo_predict(A, y, th, nu_draws=nd)
    nd[7] = 2000.0
    with pytest.raises(ValueError, match="between 0.06 and 1000"):
        pybmc_amd.psis_loo_predict(A, y, th, nu_draws=nd)
    with pytest.raises(ValueError, match="nu_draws must be shaped"):
        pybmc_amd.psis_loo_predict(A, y, th, nu_draws=np.full(24, 4.0))


def test_loo_predictions_routes_the_three_kinds_of_fit(monkeypatch):
    """loo_predictions() hands the fit's own likelihood on; loo_predict() keeps refusing a t fit."""
    import pandas as pd
    from pybmc_amd import scoring
    from pybmc_amd.bmc import BayesianModelCombination
    df = pd.DataFrame({"N": [1, 2, 3], "Z": [1, 1, 2], "a": [1.0, 2.0, 3.0], "b": [1.5, 2.5, 2.0],
                       "truth": [1.2, 2.2, 2.6]})
    bmc = BayesianModelCombination(["a", "b"], {"p": df}, "truth")
    with pytest.raises(ValueError, match="train"):
        bmc.loo_predictions()
    bmc.samples = np.zeros((4, 2))
    bmc.U_hat = np.ones((3, 1))
    bmc.Vt_hat = np.ones((1, 2))
    bmc.S_hat = np.ones(1)
    bmc.centered_experiment_train = np.array([0.1, 0.2, 0.3])
    bmc._predictions_mean_train = np.array([1.0, 2.0, 3.0])
    bmc.n_chains = 2
    seen = []

    def fake(A, y, samples, burn=0, thin=1, device=0, nu=None, nu_draws=None):
        seen.append((np.asarray(A).shape, np.asarray(samples).shape, burn, nu,
                     None if nu_draws is None else np.asarray(nu_draws).tolist()))
        return {"loo_mean": np.array([0.0, 0.1, 0.2]), "loo_pit": np.full(3, 0.5)}

    monkeypatch.setattr(scoring, "psis_loo_predict", fake)
    bmc._trained_with = ("gibbs", [np.zeros(1), np.eye(1), 1.0, 0.02])
    g = bmc.loo_predictions()
    assert g["likelihood"] == "gaussian" and g["nu"] is None and "nu_estimated" not in g
    np.testing.assert_allclose(g["predicted"], [1.0, 2.1, 3.2])
    np.testing.assert_allclose(g["residual"], [0.1, 0.1, 0.1])
    np.testing.assert_allclose(g["truth"], [1.1, 2.2, 3.3])
    bmc._trained_with = ("student_t", [np.zeros(1), np.eye(1), 1.0, 0.02], 4.0)
    t = bmc.loo_predictions(burn=1)
    assert t["likelihood"] == "student_t" and t["nu"] == 4.0
    with pytest.raises(ValueError, match="supports the Gaussian Gibbs sampler only"):
        bmc.loo_predict()
    bmc._trained_with = ("student_t", [np.zeros(1), np.eye(1), 1.0, 0.02], "estimate")
    bmc.nu_samples = np.array([3.0, 5.0, 7.0, 9.0])
    e = bmc.loo_predictions(burn=1)
    assert e["likelihood"] == "student_t" and e["nu_estimated"] is True and e["nu"] == 7.0
    with pytest.raises(ValueError, match="supports the Gaussian Gibbs sampler only"):
        bmc.loo_predict()
    assert seen == [((3, 1), (2, 2, 2), 0, None, None), ((3, 1), (2, 2, 2), 1, 4.0, None),
                    ((3, 1), (2, 2, 2), 1, None, [[3.0, 5.0], [7.0, 9.0]])]


# ---- the C ABI ------------------------------------------------------------------------------------------
def test_new_entry_points_are_bound_and_refuse_null():
    import re
    from pybmc_amd import _lib
    header = open(os.path.join(HERE, "..", "include", "pybmc_amd.h")).read()
    assert "#define PYBMC_AMD_ABI_VERSION 4" in header             # additive
    for kind in ("t", "tv"):
        for suffix in ("", "_device"):
            name = f"bmc_psis_loo_predict_{kind}{suffix}"
            new = re.search(rf"int {name}\(([^;]*)\);", header)
            base = re.search(rf"int bmc_psis_loo_{kind}{suffix}\(([^;]*)\);", header)
            assert new and base, name
            npar = [p.strip() for p in new.group(1).replace("\n", " ").split(",")]
            bpar = [p.strip() for p in base.group(1).replace("\n", " ").split(",")]
            assert npar[:len(bpar)] == bpar and len(npar) == len(bpar) + 4
            assert [p.split("*")[-1].strip() for p in npar[-4:]] == ["loo_mean_out", "loo_sd_out",
                                                                     "loo_pit_out", "ess_out"]
            assert len(_lib.PROTOTYPES[name][1]) == len(npar)
            assert callable(getattr(_lib.Context, name[4:]))
    lib = _lib.load_library()
    # a NULL context is refused before anything touches a device
    head = (None, None, 1, 1, 1, 0, None, None, 2, 2)
    assert lib.bmc_psis_loo_predict_t(*head, 4.0, *(None,) * 7) == 1
    assert lib.bmc_psis_loo_predict_t_device(*head, 4.0, *(None,) * 7) == 1
    assert lib.bmc_psis_loo_predict_tv(*head, None, 1, None, *(None,) * 7) == 1
    assert lib.bmc_psis_loo_predict_tv_device(*head, None, 1, None, *(None,) * 7) == 1
