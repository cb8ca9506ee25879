"""The Student-t scores without a GPU: log1p_nonneg of bmc_math.h against libm, the numpy reference
of tests/tscore_reference.py against scipy and against its own long-double run, compare_elpd, the
``nu`` checks of the three scoring functions and the dispatch of BayesianModelCombination.score."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import pybmc_amd
from pybmc_amd import _lib, scoring

import tscore_reference as T

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "pybmc_amd.h")


def test_log1p_nonneg_against_libm(tmp_path):
    """g++ builds tests/tscore_math_check.cpp from the text the kernels compile.  Bar: 2.01 ulp, the
    bar test_host_math.py sets for this header's sin and cos.  Measured worst case over 3 000 000
    arguments of each family: 0.7358 ulp (10^U(-320, 300)), 0.8164 ulp (U(0, 4), at x = 0.407),
    0.7656 ulp (2^U(-60, 10)); 0, 0.25, 0.21 and 0.21 ulp at 0, 2^-53, 1 and DBL_MAX."""
    exe = tmp_path / "tscore_math_check"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o", str(exe),
                    os.path.join(HERE, "tscore_math_check.cpp")], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    print(out)
    worst = [float(v) for v in out[0].split()]
    assert len(worst) == 3 and max(worst) <= 2.01, worst
    values = [tuple(float(v) for v in line.split()) for line in out[1:5]]
    assert values[0] == (0.0, 0.0)                         # log1p(0) is 0, exactly
    assert values[1][0] == 2.0 ** -53                      # below half an ulp of 1: x itself
    assert all(err <= 2.01 for _, err in values), values
    assert values[3][0] == pytest.approx(709.782712893384, rel=1e-15)   # DBL_MAX: no overflow
    is_nan, inf_is_finite = (int(v) for v in out[5].split())
    assert is_nan == 1 and inf_is_finite == 0


def test_reference_agrees_with_scipy():
    """Bar 1e-13 of max(1, |ll|); measured 1.0e-14."""
    from scipy import stats
    worst = 0.0
    for nu in T.NUS:
        for make in (lambda: T.shape_case(5, 65, 513), T.outlier_case, T.tiny_case):
            A, y, th = make()
            ll = T.loglik_t(A, y, th, nu)
            r = y[:, None] - A @ th[:, :-1].T
            want = stats.t.logpdf(r / th[:, -1][None, :], nu) - np.log(th[:, -1])[None, :]
            worst = max(worst, float(np.max(np.abs(ll - want) / np.maximum(1.0, np.abs(want)))))
    print(f"reference against scipy.stats.t.logpdf: {worst:.3e}")
    assert worst <= 1e-13


def test_reference_rounding_floor():
    """The float64 reference against its long-double run over exactly the cases of
    test_tscore_gpu.py: every floor must stay under 1/100 of its bar (a case that breaks this is
    changed, the bar is not).  Measured: lppd 1.6e-15, p_waic 1.8e-15, mean_ll 4.2e-16,
    elpd_loo_i 1.7e-15, pareto_k 2.5e-14."""
    worst = {}
    for tag, kind, key in T.all_cases():
        A, y, th = T.case_arrays(kind, key)
        for nu in T.NUS:
            wide = (T.pointwise(A, y, th, nu, np.longdouble), T.loo_pointwise(A, y, th, nu, np.longdouble))
            for name, v in T.deviations(T.reference(kind, key, nu), *wide).items():
                if v > worst.get(name, (0.0,))[0]:
                    worst[name] = (v, tag, nu)
    print(worst)
    bars = {"lppd": T.BAR_LPPD, "loo_lppd": T.BAR_LPPD, "p_waic": T.BAR_REL, "mean_ll": T.BAR_REL,
            "elpd_loo": T.BAR_ELPD, "pareto_k": T.BAR_K}
    for name, bar in bars.items():
        assert worst[name][0] <= bar / 100, (name, worst[name])


def test_the_tiny_case_is_tiny_and_the_outlier_large():
    A, y, th = T.tiny_case()
    r = y[:, None] - A @ th[:, :-1].T
    assert np.array_equal(r, np.repeat(y[:, None], len(th), 1)) and r.min() == 1e-20
    x = r * r / (4.0 * th[:, -1] ** 2)[None, :]
    assert x.min() < 1e-40 and np.all(np.log(1.0 + x[x < 1e-17]) == 0.0)   # what a naive log gives
    A, y, th = T.outlier_case()
    r0 = y[0] - A[0] @ th[:, :-1].T
    assert np.min(r0 * r0 / (1.5 * th[:, -1] ** 2)) > 400


# ---- compare_elpd ------------------------------------------------------------------------------------
def _loo_result(v):
    return {"elpd_loo_i": np.asarray(v, dtype=np.float64), "elpd_loo": float(np.sum(v))}


def test_compare_elpd_arithmetic_and_order():
    assert "compare_elpd" in pybmc_amd.__all__
    rng = np.random.default_rng(3)
    n = 57
    a, b, c = rng.standard_normal((3, n))
    b = b + 0.4
    out = pybmc_amd.compare_elpd({"a": _loo_result(a), "b": _loo_result(b), "c": _loo_result(c)})
    sums = {"a": a.sum(), "b": b.sum(), "c": c.sum()}
    vec = {"a": a, "b": b, "c": c}
    want = sorted(sums, key=lambda m: -sums[m])
    assert out["names"] == want and out["kind"] == "elpd_loo_i" and out["n_points"] == n
    best = vec[want[0]]
    for j, m in enumerate(want):
        assert out["elpd"][j] == pytest.approx(sums[m], rel=1e-14)
        assert out["se"][j] == pytest.approx(np.sqrt(n * np.var(vec[m], ddof=1)), rel=1e-14)
        assert out["elpd_diff"][j] == pytest.approx(sums[want[0]] - sums[m], rel=1e-13, abs=1e-13)
        want_se = 0.0 if j == 0 else np.sqrt(n * np.var(best - vec[m], ddof=1))
        assert out["se_diff"][j] == pytest.approx(want_se, rel=1e-14)
    assert out["elpd_diff"][0] == 0.0 and out["se_diff"][0] == 0.0
    # the formula of cv.path_summary
    ps = pybmc_amd.path_summary(np.arange(1, 4), np.stack([a, b, c]))
    back = [want.index(m) for m in ("a", "b", "c")]
    np.testing.assert_allclose(out["elpd_diff"][back], ps["elpd_diff"], rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(out["se_diff"][back], ps["se_diff"], rtol=1e-13)
    # ties keep the input order
    tie = pybmc_amd.compare_elpd({"z": _loo_result(a), "y": _loo_result(a.copy()), "x": _loo_result(a - 1)})
    assert tie["names"] == ["z", "y", "x"] and tie["se_diff"][1] == 0.0
    # the other kinds
    w = pybmc_amd.compare_elpd({"p": {"elpd_waic_i": a, "elpd_waic": a.sum(), "lppd": a + 1},
                                "q": {"elpd_waic_i": b, "elpd_waic": b.sum(), "lppd": b + 1}})
    assert w["kind"] == "elpd_waic_i" and w["names"] == ["q", "p"]
    assert pybmc_amd.compare_elpd({"p": {"elpd_cv_i": a, "elpd_cv": a.sum()}})["kind"] == "elpd_cv_i"
    assert pybmc_amd.compare_elpd({"p": {"lppd": a, "elpd": a.sum()}})["kind"] == "lppd"
    # NaNs propagate
    bad = a.copy()
    bad[5] = np.nan
    nn = pybmc_amd.compare_elpd({"good": _loo_result(a), "bad": _loo_result(bad)})
    assert nn["names"] == ["good", "bad"] and np.isnan(nn["elpd"][1]) and np.isnan(nn["se_diff"][1])
    assert np.isnan(nn["elpd_diff"][1]) and nn["elpd"][0] == pytest.approx(a.sum())


def test_compare_elpd_refusals():
    a = np.arange(5.0)
    for fits in ({}, [], {"a": a}, {"a": {"elpd_loo_i": a}},
                 {"a": _loo_result(a), "b": {"elpd_waic_i": a, "elpd_waic": 1.0}},
                 {"a": _loo_result(a), "b": _loo_result(np.arange(6.0))},
                 {"a": _loo_result(a.reshape(5, 1))}):
        with pytest.raises(ValueError):
            pybmc_amd.compare_elpd(fits)


# ---- nu= of the scoring functions ----------------------------------------------------------------------
def test_nu_is_checked_before_any_device_work(monkeypatch):
    def no_device(*a, **kw):
        raise AssertionError("argument errors must be raised before any device work")

    monkeypatch.setattr(_lib, "default_context", no_device)
    A, y, th = T.shape_case(4, 63, 25)
    for f in (pybmc_amd.pointwise_log_likelihood, pybmc_amd.waic, pybmc_amd.psis_loo):
        for nu in (0, 0.0, -1.0, float("nan"), float("inf"), -float("inf"), "4", True, [4.0]):
            with pytest.raises(ValueError, match="nu must be"):
                f(A, y, th, nu=nu)


def test_nu_selects_the_t_entry_points(monkeypatch):
    calls = []

    class Ctx:
        lock = threading.RLock()

        def __getattr__(self, name):
            def call(*a):
                calls.append((name, a[9:]))
                n = a[1]
                return {key: np.zeros(n) for key in ("lppd", "p_waic", "mean_ll", "elpd_loo", "pareto_k")}
            return call

    monkeypatch.setattr(_lib, "default_context", lambda device=0: Ctx())
    A, y, th = T.shape_case(4, 63, 25)
    pybmc_amd.pointwise_log_likelihood(A, y, th)
    pybmc_amd.pointwise_log_likelihood(A, y, th, nu=4)
    pybmc_amd.waic(A, y, th, nu=np.float64(1.5))
    pybmc_amd.psis_loo(A, y, th, nu=None)
    pybmc_amd.psis_loo(A, y, th, nu=50.0)
    assert calls == [("pointwise_loglik", ()), ("pointwise_loglik_t", (4.0,)),
                     ("pointwise_loglik_t", (1.5,)), ("psis_loo", ()), ("psis_loo_t", (50.0,))]


def test_header_declares_and_python_binds_the_entry_points():
    with open(HEADER) as fh:
        text = fh.read()
    assert "#define PYBMC_AMD_ABI_VERSION 4" in text          # additive
    for name in ("bmc_pointwise_loglik", "bmc_psis_loo"):
        for suffix in ("", "_device"):
            plain = re.search(rf"int {name}{suffix}\(([^;]*)\);", text)
            t = re.search(rf"int {name}_t{suffix}\(([^;]*)\);", text)
            assert plain and t, name + suffix
            pp = [p.strip() for p in plain.group(1).replace("\n", " ").split(",")]
            tp = [p.strip() for p in t.group(1).replace("\n", " ").split(",")]
            assert tp[:10] == pp[:10] and tp[10] == "double nu" and tp[11:] == pp[10:]
            assert "ldt" in tp[9]
            assert len(_lib.PROTOTYPES[f"{name}_t{suffix}"][1]) == len(tp)
            assert hasattr(_lib.Context, f"{name[4:]}_t{suffix}")
    lib = _lib.load_library()
    assert all(hasattr(lib, n) for n in ("bmc_pointwise_loglik_t", "bmc_pointwise_loglik_t_device",
                                         "bmc_psis_loo_t", "bmc_psis_loo_t_device"))


# ---- BayesianModelCombination.score ---------------------------------------------------------------------
def test_score_dispatch(monkeypatch):
    """score() hands the fit's own likelihood on: nu after "student_t", None otherwise; the old
    methods keep refusing a Student-t fit."""
    import pandas as pd
    from pybmc_amd.bmc import BayesianModelCombination
    df = pd.DataFrame({"N": [1, 2, 3], "Z": [1, 1, 2], "a": [1.0, 2.0, 3.0], "b": [1.5, 2.5, 2.0],
                       "truth": [1.2, 2.2, 2.6]})
    bmc = BayesianModelCombination(["a", "b"], {"p": df}, "truth")
    with pytest.raises(ValueError, match="train"):
        bmc.score()
    bmc.samples = np.zeros((4, 2))
    bmc.U_hat = np.ones((3, 1))
    bmc.Vt_hat = np.ones((1, 2))
    bmc.S_hat = np.ones(1)
    bmc.centered_experiment_train = np.zeros(3)
    bmc.n_chains = 2
    seen = []

    def fake(name, result):
        def f(A, y, samples, burn=0, thin=1, device=0, nu=None):
            seen.append((name, np.asarray(A).shape, np.asarray(samples).shape, burn, nu))
            return dict(result)
        return f

    monkeypatch.setattr(scoring, "psis_loo", fake("loo", {"elpd_loo": 1.0, "elpd_loo_i": np.ones(3)}))
    monkeypatch.setattr(scoring, "waic", fake("waic", {"elpd_waic": 1.0, "elpd_waic_i": np.ones(3)}))
    monkeypatch.setattr(scoring, "pointwise_log_likelihood", fake("pw", {"lppd": np.ones(3)}))

    bmc._trained_with = ("gibbs", [np.zeros(1), np.eye(1), 1.0, 0.02])
    g = bmc.score()
    assert g["likelihood"] == "gaussian" and g["nu"] is None and g["elpd_loo"] == 1.0
    bmc._trained_with = ("student_t", [np.zeros(1), np.eye(1), 1.0, 0.02], 4.0)
    t = bmc.score("loo", burn=1)
    assert t["likelihood"] == "student_t" and t["nu"] == 4.0
    w = bmc.score(method="waic")
    assert w["likelihood"] == "student_t" and "elpd_waic_i" in w
    h = bmc.score(X=df[["a", "b", "truth"]])
    assert h["likelihood"] == "student_t" and h["nu"] == 4.0 and h["elpd"] == 3.0 and h["n_points"] == 3
    assert seen == [("loo", (3, 1), (2, 2, 2), 0, None), ("loo", (3, 1), (2, 2, 2), 1, 4.0),
                    ("waic", (3, 1), (2, 2, 2), 0, 4.0), ("pw", (3, 1), (2, 2, 2), 0, 4.0)]
    assert pybmc_amd.compare_elpd({"gauss": g, "t": t})["names"] == ["gauss", "t"]   # feeds it directly
    with pytest.raises(ValueError, match="method must be"):
        bmc.score("kfold")
    with pytest.raises(ValueError, match="DataFrame"):
        bmc.score(X=df.values)
    with pytest.raises(ValueError, match="truth"):
        bmc.score(X=df[["a", "b"]])
    for call in (bmc.waic, bmc.loo, bmc.loo_predict):
        with pytest.raises(ValueError, match="supports the Gaussian Gibbs sampler only"):
            call()
