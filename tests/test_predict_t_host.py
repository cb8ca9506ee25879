"""The device-made Student-t noise of predict() / evaluate() without a GPU: the header and the
binding, the ninth stream and its (point, draw) counter rule, the restatement of
tests/predict_t_reference.py against scipy's t distribution and against the CPU build of bmc_math.h's
student_t_variate (tests/predict_t_math_check.cpp), the independence that one counter per entry buys,
and the surface: the argument checks of Context.predict and the ``noise_source`` keyword of
sampling_utils and of BayesianModelCombination."""
import os
import re
import threading

import numpy as np
import pytest
import scipy.stats

from pybmc_amd import _lib, sampling_utils

import predict_t_host_build as H
import predict_t_reference as PT

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "pybmc_amd.h")
BMC_DEV = os.path.join(ROOT, "pybmc_amd", "csrc", "bmc_dev.h")


# ---- header, binding, stream ----------------------------------------------------------------------
def test_header_keeps_abi_4_and_declares_both_entry_points():
    text = open(HEADER).read()
    assert re.search(r"#define\s+PYBMC_AMD_ABI_VERSION\s+4\b", text)
    assert _lib.ABI_VERSION == 4
    for name in ("bmc_predict_t", "bmc_predict_tv"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text)
        assert name in _lib.PROTOTYPES
    # bmc_predict's arguments without rng_mode and noise, and the degrees of freedom behind them
    base = list(_lib.PROTOTYPES["bmc_predict"][1])
    del base[10], base[8]
    assert _lib.PROTOTYPES["bmc_predict_t"][1][:-1] == base
    assert _lib.PROTOTYPES["bmc_predict_tv"][1][:-1] == base
    assert _lib.PROTOTYPES["bmc_predict_t"][1][-1] is _lib.C.c_double
    assert _lib.PROTOTYPES["bmc_predict_tv"][1][-1] is _lib.PROTOTYPES["bmc_predict"][1][1]


def test_the_stream_constant_is_new():
    text = open(BMC_DEV).read()
    streams = {n: int(v, 16) for n, v in re.findall(r"\b(STREAM_[A-Z_]+)\s*=\s*(0x[0-9a-fA-F]+)u", text)}
    assert len(streams) == 9
    assert streams["STREAM_PRED_T"] == PT.STREAM_PRED_T == int.from_bytes(b"PRET", "big")
    others = [v for n, v in streams.items() if n != "STREAM_PRED_T"]
    assert len(set(others)) == 8 and PT.STREAM_PRED_T not in others


@pytest.mark.parametrize("M,S", [(13, 100), (130, 1000)])
def test_the_counter_map_is_injective(M, S):
    e = PT.counter_index(S, M)
    assert e.shape == (S, M)
    assert len(np.unique(e)) == M * S
    assert int(e[S - 1, M - 1]) == (M - 1) * S + S - 1 and int(e[3, 2]) == 2 * S + 3


# ---- z[p, s] depends on (seed, p, s, nu_s) alone --------------------------------------------------
def test_noise_depends_on_seed_point_draw_and_nu_alone():
    seed, S = PT.SEEDS[1], 100
    z13 = PT.noise(seed, S, 13, PT.CYCLE)
    z7 = PT.noise(seed, S, 7, PT.CYCLE)
    assert np.array_equal(z13[:, :7], z7)
    nus = PT.nu_of_draws(PT.CYCLE, S)
    other = nus.copy()
    other[37] = 50.0 if nus[37] != 50.0 else 4.0
    moved = PT.noise(seed, S, 13, other) != z13
    assert moved[37].all() and not np.delete(moved, 37, axis=0).any()
    # one value per draw, all equal, is the one-nu matrix
    assert np.array_equal(PT.noise(seed, S, 13, np.full(S, 4.0)), PT.noise(seed, S, 13, 4.0))
    assert not np.array_equal(PT.noise(PT.SEEDS[0], S, 13, 4.0), PT.noise(seed, S, 13, 4.0))


# ---- the CPU build of the variate on this stream's uniforms ------------------------------------
@pytest.mark.parametrize("nu", PT.NUS)
def test_cpu_build_stays_within_the_recorded_accuracy(nu):
    for seed in PT.SEEDS:
        ref = PT.noise(seed, 1000, 130, nu)
        cpu = H.noise(seed, 1000, 130, nu)
        worst = float((np.abs(cpu.astype(PT.LD) - ref) / np.abs(ref)).max())
        print(f"nu {nu} seed {seed}: {worst / 2.0 ** -52:.2f} units of 2^-52 |t| "
              f"(bar {PT.T_ACCURACY[nu] / 2.0 ** -52:.1f})")
        assert worst <= PT.T_ACCURACY[nu]


# ---- the distribution, and the independence of points p and p + 4 -----------------------------
@pytest.mark.parametrize("nu", [1.5, 4.0])
@pytest.mark.parametrize("seed", PT.SEEDS)
def test_restated_noise_is_t_distributed(seed, nu):
    z = PT.noise(seed, 10000, 8, nu).astype(np.float64)
    p_all = scipy.stats.kstest(z.ravel(), scipy.stats.t(nu).cdf).pvalue
    p_pts = [scipy.stats.kstest(z[:, p], scipy.stats.t(nu).cdf).pvalue for p in range(8)]
    print(f"nu {nu} seed {seed}: KS p {p_all:.4f} over all, smallest per point {min(p_pts):.4f}")
    assert p_all > 1e-4 and min(p_pts) > 1e-4


@pytest.mark.parametrize("nu", [1.5, 4.0])
@pytest.mark.parametrize("seed", PT.SEEDS)
def test_points_four_apart_do_not_share_a_radius(seed, nu):
    """u = cdf(|z|) of points p and p + 4 correlate below 6 / sqrt(S).  Were the sine half of a
    counter handed to point p + 4, as the Gaussian walk hands it, the two would share a radius and
    correlate at about 0.8 (nu = 1.5): the second half of this test builds that matrix and sees it
    fail the bar."""
    S = 10000
    z = PT.noise(seed, S, 8, nu).astype(np.float64)
    u = scipy.stats.t.cdf(np.abs(z), nu)
    corr = [abs(np.corrcoef(u[:, p], u[:, p + 4])[0, 1]) for p in range(4)]
    print(f"nu {nu} seed {seed}: |corr| of points p, p + 4: " + " ".join(f"{c:.4f}" for c in corr))
    assert max(corr) < 6 / np.sqrt(S)
    u1, u2 = PT.uniforms(seed, S, 8)
    import ppc_t_reference as T
    cs, sn = T.t_variate(u1[:, :4], u2[:, :4], nu)
    us = scipy.stats.t.cdf(np.abs(np.concatenate([cs, sn], axis=1).astype(np.float64)), nu)
    shared = [abs(np.corrcoef(us[:, p], us[:, p + 4])[0, 1]) for p in range(4)]
    assert min(shared) > 6 / np.sqrt(S)


# ---- argument checks, before any library call ------------------------------------------------------
class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} reached")


def bare_context():
    ctx = object.__new__(_lib.Context)
    ctx._lib = NoLibrary()
    ctx._h = None
    ctx._last_predict = None
    return ctx


def test_context_predict_checks_its_noise_arguments_first():
    ctx = bare_context()
    rng = np.random.default_rng(0)
    preds, theta, Vt = rng.standard_normal((5, 3)), np.abs(rng.standard_normal((6, 3))), np.ones((2, 3))
    for bad in ({"nu": 0.05}, {"nu": np.inf}, {"nu": np.nan}, {"nu": -1.0}, {"nu": [4.0, 4.0]},
                {"nu_draws": np.full(5, 4.0)}, {"nu_draws": np.full((6, 2), 4.0)},
                {"nu_draws": np.array([4.0, 4.0, 0.05, 4.0, 4.0, 4.0])},
                {"nu_draws": np.array([4.0, 4.0, np.inf, 4.0, 4.0, 4.0])},
                {"noise": np.zeros((6, 5)), "nu": 4.0},
                {"noise": np.zeros((6, 5)), "nu_draws": np.full(6, 4.0)},
                {"nu": 4.0, "nu_draws": np.full(6, 4.0)}):
        with pytest.raises(ValueError):
            ctx.predict(preds, theta, Vt, seed=1, **bad)
    # a good call gets past the checks, to the library
    for good in ({"nu": 0.06}, {"nu_draws": np.full((6, 1), 4.0)}):
        with pytest.raises(AssertionError, match="library call bmc_predict_t"):
            ctx.predict(preds, theta, Vt, seed=1, **good)


class FakeContext:
    """Stands where _lib.default_context's context stands: records what predict() is handed."""

    def __init__(self):
        self.lock = threading.Lock()
        self.calls = []

    def predict(self, preds, theta, Vt_hat, seed=0, noise=None, q=(2.5, 50, 97.5), truth=None,
                cov_percentiles=None, want_draws=True, draws_order="C", nu=None, nu_draws=None):
        self.calls.append({"theta": theta, "seed": seed, "noise": noise, "nu": nu, "nu_draws": nu_draws})
        M, S = np.shape(preds)[0], theta.shape[0]
        return np.zeros((S, M)), np.zeros((len(q), M)), ([0.0] * len(cov_percentiles) if truth is not None else None)


def problem():
    rng = np.random.default_rng(5)
    samples = np.column_stack([rng.standard_normal((10050, 2)), rng.uniform(0.5, 1.5, 10050)])
    return rng.standard_normal((3, 4)), samples, rng.standard_normal((2, 4)), rng.standard_normal(3)


def test_noise_source_is_checked_before_any_library_call(monkeypatch):
    def no_context(device=0):
        raise AssertionError("default_context reached")
    monkeypatch.setattr(_lib, "default_context", no_context)
    preds, samples, Vt, truth = problem()
    for src in ("gpu", "Device", None):
        with pytest.raises(ValueError, match="noise_source"):
            sampling_utils.rndm_m_random_calculator(preds, samples, Vt, seed=1, noise_df=4.0, noise_source=src)
        with pytest.raises(ValueError, match="noise_source"):
            sampling_utils.predictive_coverage([50], preds, samples, Vt, truth, seed=1, noise_df=4.0,
                                               noise_source=src)


@pytest.mark.parametrize("per_row", [False, True])
def test_device_noise_dispatch(monkeypatch, per_row):
    """With "device" the context gets nu= / nu_draws= (the chosen rows' values) and no noise array,
    Generator.standard_t is never called, and the chosen theta is the host path's."""
    fake = FakeContext()
    monkeypatch.setattr(_lib, "default_context", lambda device=0: fake)
    preds, samples, Vt, truth = problem()
    df = 2.0 + np.arange(samples.shape[0]) % 7 if per_row else 4.0
    seed = 77
    sampling_utils.rndm_m_random_calculator(preds, samples, Vt, seed=seed, noise_df=df)
    sampling_utils.predictive_coverage([50, 90], preds, samples, Vt, truth, seed=seed, noise_df=df)
    host = list(fake.calls)
    del fake.calls[:]

    def no_standard_t(self, *a, **k):
        raise AssertionError("standard_t called")
    monkeypatch.setattr(sampling_utils, "_t_noise", no_standard_t)
    sampling_utils.rndm_m_random_calculator(preds, samples, Vt, seed=seed, noise_df=df, noise_source="device")
    sampling_utils.predictive_coverage([50, 90], preds, samples, Vt, truth, seed=seed, noise_df=df,
                                       noise_source="device")
    assert len(fake.calls) == 2 and len(host) == 2
    rng = np.random.Generator(np.random.PCG64(seed))
    if per_row:
        both = rng.choice(np.column_stack([samples, df]), 10000, replace=False)
        want_theta, want_nu = both[:, :-1], both[:, -1]
    else:
        want_theta, want_nu = rng.choice(samples, 10000, replace=False), 4.0
    for dev, hst in zip(fake.calls, host):
        assert dev["noise"] is None and dev["seed"] == seed
        assert hst["noise"].shape == (10000, 3) and hst["nu"] is None and hst["nu_draws"] is None
        assert np.array_equal(dev["theta"], hst["theta"]) and np.array_equal(dev["theta"], want_theta)
        if per_row:
            assert dev["nu"] is None and dev["nu_draws"].shape == (10000,)
            assert np.array_equal(dev["nu_draws"], want_nu)
        else:
            assert dev["nu"] == 4.0 and dev["nu_draws"] is None
    # the keyword is ignored for normal noise
    del fake.calls[:]
    sampling_utils.rndm_m_random_calculator(preds, samples, Vt, seed=seed, noise_source="device")
    assert fake.calls[0]["noise"] is None and fake.calls[0]["nu"] is None and fake.calls[0]["nu_draws"] is None


def test_standard_t_is_the_host_path_only(monkeypatch):
    """The generator's standard_t itself: called on the host path, never on the device path."""
    fake = FakeContext()
    monkeypatch.setattr(_lib, "default_context", lambda device=0: fake)
    calls = []
    real = np.random.Generator

    class Spy:
        def __init__(self, bitgen):
            self._g = real(bitgen)

        def choice(self, *a, **k):
            return self._g.choice(*a, **k)

        def standard_t(self, *a, **k):
            calls.append(a)
            return self._g.standard_t(*a, **k)
    monkeypatch.setattr(sampling_utils.np.random, "Generator", Spy)
    preds, samples, Vt, _ = problem()
    sampling_utils.rndm_m_random_calculator(preds, samples, Vt, seed=3, noise_df=4.0, noise_source="device")
    assert calls == []
    sampling_utils.rndm_m_random_calculator(preds, samples, Vt, seed=3, noise_df=4.0)
    assert len(calls) == 1


def test_predict_predict2_and_evaluate_pass_the_keyword_on(monkeypatch):
    import pandas as pd
    from pybmc_amd import bmc as bmc_module
    from pybmc_amd.bmc import BayesianModelCombination
    df = pd.DataFrame({"N": [1, 2, 3], "Z": [1, 1, 2], "a": [1.0, 2.0, 3.0], "b": [1.5, 2.5, 2.0],
                       "truth": [1.2, 2.2, 2.6]})
    b = BayesianModelCombination(["a", "b"], {"p": df}, "truth")
    b.samples = np.ones((6, 2))
    b.Vt_hat = np.ones((1, 2))
    b.current_property = "p"
    b._trained_with = ("student_t", None, 4.0)
    seen = []

    def fake_calc(preds, samples, Vt_hat, **kw):
        seen.append(("calc", kw))
        return np.zeros((10000, 3)), [np.zeros(3)] * 3

    def fake_cov(pct, preds, samples, Vt_hat, truth, **kw):
        seen.append(("cov", kw))
        return [0.0] * len(pct)
    monkeypatch.setattr(bmc_module, "rndm_m_random_calculator", fake_calc)
    monkeypatch.setattr(bmc_module, "predictive_coverage", fake_cov)
    for src in ("host", "device"):
        del seen[:]
        b.predict(df[["a", "b", "N", "Z"]], noise_source=src)
        b.predict2("p", noise_source=src)
        b.evaluate(noise_source=src)
        assert [s[0] for s in seen] == ["calc", "calc", "cov"]
        assert all(s[1]["noise_source"] == src and s[1]["noise_df"] == 4.0 for s in seen)
    del seen[:]
    b.predict(df[["a", "b", "N", "Z"]])
    b.predict2("p")
    b.evaluate()
    assert all(s[1]["noise_source"] == "host" for s in seen) and len(seen) == 3


def test_the_follow_up_note_is_gone():
    text = open(os.path.join(ROOT, "pybmc_amd", "sampling_utils.py")).read()
    assert "follow-up" not in text
