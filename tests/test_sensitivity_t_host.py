"""The surface of the Student-t power-scaling sensitivity without a GPU: which entry point a call
reaches and with what table, index and log prior (a fake context, as tests/test_ppc_t_host.py), the
dispatch of BayesianModelCombination.sensitivity, the argument errors, the header."""
import os
import re
import threading

import numpy as np
import pytest

import sens_reference as SR
from pybmc_amd import _lib, sensitivity
from pybmc_amd.inference_utils import robust_nu_prior

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "pybmc_amd.h")


class FakeContext:
    """Stands where _lib.default_context's context stands: records the entry point and what it got
    behind want_weights, and returns a result of the right shapes."""

    def __init__(self):
        self.lock = threading.Lock()
        self.calls = []

    def _record(self, name, rows, nu_col, A, n, k, lda, layout, y, theta, n_draws, ldt, prior, Vt, alphas, mask,
                cpb, want_weights, *lik):
        self.calls.append((name, int(n), int(n_draws), mask, lik))
        nc, na = bin(mask).count("1"), len(alphas)
        Q = k + 1 + (0 if Vt is None else Vt.shape[1]) + nu_col
        z = np.zeros((nc, na, Q))
        return {"logdens": np.arange(rows * n_draws, dtype=np.float64).reshape(rows, n_draws),
                "pareto_k": np.zeros((nc, na)), "mean": z, "sd": z, "cjs": z + 0.001,
                "weights": np.full((n_draws, nc * na), 1.0 / n_draws) if want_weights else None,
                "component_flags": np.zeros(nc, dtype=bool), "column_flags": np.zeros(Q, dtype=bool)}

    def power_sensitivity(self, *a):
        return self._record("power_sensitivity", 3, 0, *a)

    def power_sensitivity_t(self, *a):
        return self._record("power_sensitivity_t", 4, 0, *a)

    def power_sensitivity_tv(self, *a):
        return self._record("power_sensitivity_tv", 4, 1, *a)


@pytest.fixture
def fake(monkeypatch):
    f = FakeContext()
    monkeypatch.setattr(_lib, "default_context", lambda device=0: f)
    return f


def test_function_reaches_the_entry_point_of_its_likelihood(fake):
    A, y, theta, prior, Vt = SR.random_case(12, 2, 6, 1, n_models=2)
    g = sensitivity.power_scale_sensitivity(A, y, theta, prior, Vt)
    t = sensitivity.power_scale_sensitivity(A, y, theta, prior, Vt, nu=4)
    draws = np.array([[9.0, 2.0, 4.0], [9.0, 4.0, 2.0]])
    v = sensitivity.power_scale_sensitivity(A, y, theta.reshape(2, 3, 3), prior, Vt, burn=1, nu_draws=draws)
    grid, weight = np.array([1.0, 2.0, 4.0, 9.0]), np.array([1.0, 3.0, 4.0, 0.0])
    p = sensitivity.power_scale_sensitivity(A, y, theta.reshape(2, 3, 3), prior, Vt, burn=1, nu_draws=draws,
                                            nu_grid=grid, nu_prior=weight, components=sensitivity.T_COMPONENTS)
    assert [c[0] for c in fake.calls] == ["power_sensitivity", "power_sensitivity_t", "power_sensitivity_tv",
                                          "power_sensitivity_tv"]
    assert fake.calls[0][1:] == (12, 6, 3, ()) and fake.calls[1][1:] == (12, 6, 3, (4.0,))
    for call, mask in ((fake.calls[2], 3), (fake.calls[3], 31)):
        name, n, S, m, (values, index, log_prior) = call
        assert (n, S, m) == (12, 4, mask)
        assert list(values) == [2.0, 4.0] and list(index) == [0, 1, 1, 0] and index.dtype == np.int32
    assert fake.calls[2][4][2] is None
    assert np.array_equal(fake.calls[3][4][2], np.log(np.array([3.0, 4.0]) / 8.0))
    assert (g["likelihood"], g["nu"], g["log_prior_nu"]) == ("gaussian", None, None)
    assert (t["likelihood"], t["nu"]) == ("student_t", 4.0) and t["columns"] == g["columns"]
    assert (v["likelihood"], v["nu"]) == ("student_t", 3.0)
    assert g["columns"] == ["beta_0", "beta_1", "sigma", "omega_0", "omega_1"]
    assert v["columns"] == g["columns"] + ["nu"] == p["columns"]
    assert p["components"] == sensitivity.T_COMPONENTS and set(p["psens"]) == set(sensitivity.T_COMPONENTS)
    # log_prior = (lp_beta + lp_sigma2) + lp_nu from the four rows; the Gaussian result from its three
    lb, ls, ll, ln = np.arange(16.0).reshape(4, 4)
    assert np.array_equal(p["log_prior"], (lb + ls) + ln) and np.array_equal(p["log_prior_nu"], ln)
    assert np.array_equal(p["log_lik"], ll) and np.array_equal(g["log_prior"], np.arange(6.0) + np.arange(6.0, 12.0))
    # the table of a t result: one row per column, the nu row last, one psens column per component
    tab = sensitivity.sensitivity_summary(p)
    assert list(tab.index) == p["columns"] and list(tab.columns) == list(sensitivity.T_COMPONENTS) + ["diagnosis"]
    assert list(sensitivity.sensitivity_summary(g).columns) == ["prior", "likelihood", "diagnosis"]
    w, kh = sensitivity.power_scale_weights(A, y, theta, prior, component="likelihood", nu=2.5)
    assert fake.calls[-1][0] == "power_sensitivity_t" and fake.calls[-1][3:] == (2, (2.5,)) and w.shape == (6,)
    sensitivity.power_scale_weights(A, y, theta, prior, component="prior_nu", nu_draws=np.full(6, 2.0),
                                    nu_grid=[2.0], nu_prior=[1.0])
    assert fake.calls[-1][0] == "power_sensitivity_tv" and fake.calls[-1][3] == 16
    assert list(fake.calls[-1][4][2]) == [0.0]


def test_argument_errors(fake):
    A, y, theta, prior, Vt = SR.random_case(12, 2, 6, 1, n_models=2)
    f = sensitivity.power_scale_sensitivity
    with pytest.raises(ValueError, match="not both"):
        f(A, y, theta, prior, nu=4.0, nu_draws=np.full(6, 4.0))
    for bad in (0.0, -1.0, float("inf"), float("nan"), "4", True):
        with pytest.raises(ValueError, match="nu must be None or a positive finite number"):
            f(A, y, theta, prior, nu=bad)
    with pytest.raises(ValueError, match="shaped like the leading dimensions"):
        f(A, y, theta, prior, nu_draws=np.full(5, 4.0))
    with pytest.raises(ValueError, match="nu_draws must be positive and finite"):
        f(A, y, theta, prior, nu_draws=np.r_[np.full(5, 4.0), np.nan])
    # the prior of nu belongs to nu_draws
    for kw in ({"nu_grid": [2.0, 4.0]}, {"nu_prior": [1.0, 1.0]}, {"nu": 4.0, "nu_grid": [2.0, 4.0]},
               {"nu": 4.0, "nu_prior": [1.0]}):
        with pytest.raises(ValueError, match="give nu_draws"):
            f(A, y, theta, prior, **kw)
    draws = np.array([2.0, 4.0, 4.0, 2.0, 4.0, 2.0])
    # a drawn value off the grid, a drawn value of weight 0, what robust_nu_prior refuses
    for kw in ({"nu_grid": [2.0, 5.0]}, {"nu_grid": [1.0, 2.0]}, {"nu_grid": [2.0, 4.0], "nu_prior": [1.0, 0.0]}):
        with pytest.raises(ValueError, match="value of nu_grid with a positive prior weight"):
            f(A, y, theta, prior, nu_draws=draws, **kw)
    with pytest.raises(ValueError, match="strictly increasing"):
        f(A, y, theta, prior, nu_draws=draws, nu_grid=[4.0, 2.0])
    with pytest.raises(ValueError, match="one weight per value"):
        f(A, y, theta, prior, nu_draws=draws, nu_grid=[2.0, 4.0], nu_prior=[1.0])
    # prior_nu is a component only with that prior
    for kw in ({}, {"nu": 4.0}, {"nu_draws": draws}):
        with pytest.raises(ValueError, match="prior_nu"):
            f(A, y, theta, prior, components=("prior", "prior_nu"), **kw)
        with pytest.raises(ValueError, match="prior_nu"):
            sensitivity.power_scale_weights(A, y, theta, prior, component="prior_nu", **kw)
    with pytest.raises(ValueError, match="unknown component"):
        f(A, y, theta, prior, components=("posterior",), nu_draws=draws, nu_grid=[2.0, 4.0])
    assert fake.calls == []
    # the defaults of the sampler when only one of the two is given
    grid, weight, _ = robust_nu_prior()
    f(A, y, theta, prior, nu_draws=grid[[3, 5, 5, 3, 9, 9]], nu_prior=weight, components=("prior_nu",))
    values, index, lp = fake.calls[0][4]
    assert np.array_equal(values, grid[[3, 5, 9]]) and np.array_equal(lp, np.log(weight[[3, 5, 9]] / weight.sum()))
    assert sensitivity.COMPONENTS == ("prior", "likelihood", "prior_beta", "prior_sigma2")
    assert sensitivity.T_COMPONENTS == sensitivity.COMPONENTS + ("prior_nu",)


def test_sensitivity_dispatch(fake):
    """sensitivity() reads the last fit under its own likelihood: the plain call after a Gaussian
    fit, nu= after "student_t", nu_draws= with the remembered prior after "nu": "estimate";
    ValueError after "simplex"; prior_sensitivity() keeps refusing a Student-t fit."""
    import pandas as pd
    from pybmc_amd.bmc import BayesianModelCombination
    df = pd.DataFrame({"N": [1, 2, 3], "Z": [1, 1, 2], "a": [1.0, 2.0, 3.0], "b": [1.5, 2.5, 2.0],
                       "truth": [1.2, 2.2, 2.6]})
    bmc = BayesianModelCombination(["a", "b"], {"p": df}, "truth")
    with pytest.raises(ValueError, match="train"):
        bmc.sensitivity()
    bmc.samples = np.abs(np.random.default_rng(0).standard_normal((6, 2))) + 0.1
    bmc.U_hat = np.ones((3, 1))
    bmc.Vt_hat = np.ones((1, 2))
    bmc.S_hat = np.ones(1)
    bmc.centered_experiment_train = np.array([0.1, -0.2, 0.3])
    bmc.n_chains = 2
    prior = [np.zeros(1), np.eye(1), 1.0, 0.02]

    bmc._trained_with = ("gibbs", prior)
    g = bmc.sensitivity(burn=1, alphas=[0.9])
    old = bmc.prior_sensitivity(burn=1, alphas=[0.9])
    assert [c[:4] for c in fake.calls] == [("power_sensitivity", 3, 4, 3)] * 2 and fake.calls[0][4] == ()
    assert g["likelihood"] == "gaussian" and g["columns"] == old["columns"] == ["beta_0", "sigma", "a", "b"]
    assert list(g["alphas"]) == [0.99, 1.01, 0.9]

    del fake.calls[:]
    bmc._trained_with = ("student_t", prior, 4.0)
    t = bmc.sensitivity()
    assert fake.calls == [("power_sensitivity_t", 3, 6, 3, (4.0,))]
    assert t["likelihood"] == "student_t" and t["nu"] == 4.0 and t["columns"] == g["columns"]
    tight = bmc.sensitivity(training_options={"b_mean_cov": np.eye(1) * 1e-4})
    assert tight["nu"] == 4.0 and len(fake.calls) == 2
    with pytest.raises(ValueError, match="supports the Gaussian Gibbs sampler only"):
        bmc.prior_sensitivity()

    del fake.calls[:]
    bmc._trained_with = ("student_t", prior, "estimate")
    bmc.nu_samples = np.array([2.0, 3.0, 3.0, 8.0, 2.0, 3.0])
    grid, weight = np.array([2.0, 3.0, 5.0, 8.0]), np.array([1.0, 2.0, 4.0, 1.0])
    bmc._nu_prior = (grid, weight)
    e = bmc.sensitivity(burn=1)
    name, n, S, mask, (values, index, lp) = fake.calls[0]
    assert (name, n, S, mask) == ("power_sensitivity_tv", 3, 4, 1 | 2 | 16)
    assert list(values) == [2.0, 3.0] and list(index) == [1, 1, 0, 1]
    assert np.array_equal(lp, np.log(np.array([1.0, 2.0]) / 8.0))
    assert e["columns"] == g["columns"] + ["nu"] and e["components"] == ("prior", "likelihood", "prior_nu")
    assert e["nu"] == pytest.approx(np.mean([3.0, 3.0, 2.0, 3.0])) and e["likelihood"] == "student_t"
    with pytest.raises(ValueError, match="supports the Gaussian Gibbs sampler only"):
        bmc.prior_sensitivity()

    bmc._trained_with = ("simplex", prior)
    with pytest.raises(ValueError, match="simplex"):
        bmc.sensitivity()
    bmc._trained_with = ("gibbs", prior)
    with pytest.raises(ValueError, match="simplex"):
        bmc.sensitivity(training_options={"sampler": "simplex"})


def test_train_remembers_the_prior_of_nu(monkeypatch):
    """train() keeps the grid and weights it handed the sampler; _trained_with keeps its shape."""
    import pandas as pd
    from pybmc_amd import bmc as bmc_module
    df = pd.DataFrame({"a": [1.0, 2.0, 3.0, 4.0], "b": [1.5, 2.5, 2.0, 4.5], "truth": [1.2, 2.2, 2.6, 4.1]})
    b = bmc_module.BayesianModelCombination(["a", "b"], {"p": df}, "truth")
    b.orthogonalize("p", df, components_kept=1, method="svd")
    seen = {}

    def sampler(y, X, iterations, prior, nu, **kw):
        seen.update(kw, nu=nu)
        out = (np.ones((iterations, 2)), np.ones(len(y)))
        return out + ((np.full(iterations, 3.0),) if kw["return_nu"] else ()) + ({},)

    monkeypatch.setattr(bmc_module, "gibbs_sampler_robust", sampler)
    assert b._nu_prior is None
    b.train({"iterations": 5, "sampler": "student_t", "nu": "estimate", "nu_grid": [2.0, 3.0], "nu_prior": [1.0, 3.0]})
    assert list(b._nu_prior[0]) == [2.0, 3.0] and list(b._nu_prior[1]) == [1.0, 3.0]
    assert b._trained_with[0] == "student_t" and b._trained_with[2] == "estimate" and len(b._trained_with) == 3
    b.train({"iterations": 5, "sampler": "student_t", "nu": "estimate"})
    grid, weight, _ = robust_nu_prior()
    assert np.array_equal(b._nu_prior[0], grid) and np.array_equal(b._nu_prior[1], weight)
    b.train({"iterations": 5, "sampler": "student_t", "nu": 4.0})
    assert b._nu_prior is None and b._trained_with[2] == 4.0


def test_header_and_prototypes():
    text = open(HEADER).read()
    assert re.search(r"#define\s+PYBMC_AMD_ABI_VERSION\s+4\b", text) and _lib.ABI_VERSION == 4
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    norm = lambda s: [" ".join(a.split()) for a in s.split(",")]
    args = lambda name: norm(re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1))
    for suffix in ("", "_device"):
        g, t, v = (args("bmc_power_sensitivity" + mid + suffix) for mid in ("", "_t", "_tv"))
        assert [a for a in t if a != "double nu"] == g and "double nu" in t
        extra = [a for a in v if a not in g]
        assert [a.split()[-1].lstrip("*") for a in extra] == ["nu_values", "n_values",
                                                              "d_nu_index" if suffix else "nu_index", "nu_log_prior"]
        assert [a for a in v if a in g] == g
        for mid in ("_t", "_tv"):
            name = "bmc_power_sensitivity" + mid + suffix
            assert len(_lib.PROTOTYPES[name][1]) == len(args(name))
    assert callable(_lib.Context.power_sensitivity_tv_device) and callable(_lib.Context.power_sensitivity_t_device)
    import pybmc_amd
    assert "T_COMPONENTS" in pybmc_amd.__all__ and pybmc_amd.T_COMPONENTS == sensitivity.T_COMPONENTS
    assert callable(pybmc_amd.BayesianModelCombination.sensitivity)
