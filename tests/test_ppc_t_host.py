"""The Student-t posterior predictive check without a GPU: expm1_nonneg and student_t_variate of
bmc_math.h against long double (g++ builds tests/ppc_t_math_check.cpp from the text the kernels
compile), the long-double reference of tests/ppc_t_reference.py against scipy's t distribution, the
independence that taking the cosine half alone buys, the floors and bars of tests/test_ppc_t_gpu.py,
and the surface: the ``nu`` / ``nu_draws`` checks, the dispatch of BayesianModelCombination.check,
the header and the plan."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

from pybmc_amd import _lib, ppc

import ppc_reference as P
import ppc_t_reference as T

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "pybmc_amd.h")

# expm1_nonneg against expm1l, in ulp.  Worst found 1.34 (the dense sweep 1.33, next to powers of two
# 0.66, the variate's own arguments 1.34); the bar is that with about 2 x headroom, as log1p_nonneg's
# 2.01 stands to its 0.82.  Both numbers are in the routine's comment.
EXPM1_WORST = 1.34
EXPM1_BAR = 2.7


@pytest.fixture(scope="module")
def math_lines(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ppc_t_math") / "ppc_t_math_check"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o", str(exe),
                    os.path.join(HERE, "ppc_t_math_check.cpp")], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    print(out)
    return out


def test_expm1_nonneg_against_libm(math_lines):
    worst = [float(v) for v in math_lines[0].split()]
    assert len(worst) == 3 and max(worst) <= EXPM1_BAR, worst
    assert max(worst) <= EXPM1_WORST + 0.005           # the record in bmc_math.h is of this build
    text = open(os.path.join(os.path.dirname(HERE), "pybmc_amd", "csrc", "bmc_math.h")).read()
    assert "Worst error found against expm1l: %.2f ulp" % EXPM1_WORST in text and "bar is %.1f" % EXPM1_BAR in text
    zero, near_top, top_finite, inf_710, inf_huge = math_lines[1].split()
    assert float(zero) == 0.0                           # expm1(0) is 0, exactly
    assert int(top_finite) == 1 and float(near_top) == pytest.approx(np.expm1(709.78), rel=1e-15)
    assert int(inf_710) == 1 and int(inf_huge) == 1     # beyond the double range: +inf, no garbage


def test_variate_accuracy_is_what_the_reference_records(math_lines):
    """T_ACCURACY: the relative deviation of student_t_variate from its long-double restatement per
    nu, over u1 from 2^-53 to 1.  The recorded constants cover what this build measures and are no
    more than 10 % above it (measured 4.73e-15, 1.16e-15, 4.85e-16; at nu = 1e9 4.73e-16)."""
    vals = math_lines[2].split()
    acc = [float(v) for v in vals[:4]]
    assert int(vals[4]) == 1                            # a restatement of exactly 0 met exactly 0
    for nu, got in zip(T.NUS, acc[:3]):
        assert 0 < got <= T.T_ACCURACY[nu] <= 1.1 * got, (nu, got)
    assert tuple(T.NUS) == (1.5, 4.0, 50.0) and set(T.T_ACCURACY) == set(T.NUS)
    assert acc[3] <= T.T_ACCURACY[50.0]                 # nu = 1e9 against the same restatement


def test_variate_endpoints(math_lines):
    at_one, t006, finite006, inf005 = math_lines[3].split()
    assert float(at_one) == 0.0                         # u1 = 1 gives 0
    # nu = 0.06, u1 = 2^-53: finite, and the largest |t| there is: sqrt(nu) 2^(53 / nu)
    assert int(finite006) == 1
    want = np.sqrt(P.LD(0.06)) * P.LD(2) ** (P.LD(53) / P.LD(0.06))
    assert abs(P.LD(float(t006)) / want - 1) < 5e-13    # x d / 2: x = 1225, d up to six ulp of x
    assert int(inf005) == 1                             # below about 0.052 it is past the double range
    # nu = 1e9 against Box-Muller.  t_nu is NOT the normal at any finite nu: the radii differ by
    # sqrt(expm1(x) / x) = 1 + x / 4 + O(x^2), x = 2 L / nu, L = -log u1 <= 36.8, i.e. by up to 1.8e-8
    # at nu = 1e9.  What is left after that first-order term agrees to the variate's own accuracy
    # (x^2 / 32 < 2e-16 more; measured 8.2e-16).
    left = float(math_lines[4])
    assert left <= 2 * T.T_ACCURACY[50.0] + 2e-16, left


def test_reference_variates_are_student_t():
    """200 000 variates per nu pass a KS test against scipy.stats.t at p > 1e-3 (fixed seeds), the
    cosine half and -- each on its own -- the sine half too."""
    from scipy import stats
    for j, nu in enumerate(T.NUS):
        u1, u2 = T.uniforms(1000 + j, 200, np.arange(1000))
        c, s = T.t_variate(u1, u2, nu)
        for half in (c, s):
            p = stats.kstest(half.astype(np.float64).ravel(), stats.t(nu).cdf).pvalue
            print(f"nu = {nu}: KS p = {p:.3f}")
            assert p > 1e-3, (nu, p)
        assert np.array_equal(T.noise(1000 + j, 200, np.arange(1000), nu), c)


def test_points_32_apart_are_independent():
    """|corr(|z[i, s]|, |z[i + 32, s]|)| < 0.01 over 204 800 pairs per nu.  Handing the sine half of
    point i's pair to point i + 32, as the Gaussian walk does with its Box-Muller pair, would fail
    it: the two halves share one radius (0.80 at nu = 1.5, 0.26 at nu = 4)."""
    for j, nu in enumerate(T.NUS):
        z = np.abs(T.noise(77 + j, 64, np.arange(6400), nu).astype(np.float64))
        r = np.corrcoef(z[:32].ravel(), z[32:].ravel())[0, 1]
        u1, u2 = T.uniforms(77 + j, 32, np.arange(6400))
        c, s = (np.abs(h.astype(np.float64)) for h in T.t_variate(u1, u2, nu))
        shared = np.corrcoef(np.log1p(c).ravel(), np.log1p(s).ravel())[0, 1]
        print(f"nu = {nu}: corr {r:.4f}; of the two halves of one pair (log1p) {shared:.3f}")
        assert abs(r) < 0.01, (nu, r)
        if nu <= 4:       # (towards Box-Muller the halves part: 0.02 at nu = 50)
            assert shared > 0.1, (nu, shared)
    # every element has its own counter: nothing at i + 32 depends on whether point i exists
    full = T.noise(5, 64, np.arange(3), 4.0)
    assert np.array_equal(T.noise(5, 33, np.arange(3), 4.0), full[:33])


def test_noise_depends_on_seed_point_draw_and_nu_alone():
    z = T.noise(9, 70, np.arange(130), T.case_nu(T.CYCLE, 130))
    for s in (0, 64, 65, 129):
        assert np.array_equal(T.noise(9, 70, [s], T.NUS[s % 3])[:, 0], z[:, s])
    assert not np.array_equal(T.noise(10, 70, [0], 1.5)[:, 0], z[:, 0])
    one = T.noise(9, 70, np.arange(4), np.full(4, 4.0))
    assert np.array_equal(one, T.noise(9, 70, np.arange(4), 4.0))
    # the stream is its own: not the Gaussian check's counters
    assert T.STREAM_PPC_T == 0x50504354 != P.STREAM_PPC


@pytest.mark.parametrize("group", T.GROUPS)
def test_floors_cover_what_the_references_give(group):
    """FLOORS is measured_floors() rounded up; recomputed here, none of the device in it."""
    got = T.measured_floors(group)
    print(group, " ".join("%.3g" % (v / 1e-16) for v in got))
    for name, g, f in zip(T.TEN, got, T.FLOORS[group]):
        assert g <= f <= 1.12 * g + 1e-18, (group, name, g, f)


def test_no_bar_exceeds_a_tenth_of_the_margin_floor():
    for group in T.GROUPS:
        b = T.bars(group)
        assert tuple(b) == T.TEN and all(0 < v <= T.MARGIN_FLOOR / 10 for v in b.values()), (group, b)
        assert b == {name: P.round_up_one_digit(64 * f) for name, f in zip(T.TEN, T.FLOORS[group])}
    assert T.BAR_FACTOR == 64 and T.MARGIN_FLOOR == 1e-9


def test_no_reference_statistic_sits_on_its_observed_value():
    """Every compared |T_rep - T_obs| / max(1, |T_rep|, |T_obs|) of every case is above MARGIN_FLOOR,
    ten times the widest bar: the device's p-values must equal the reference's."""
    every = [(T.case_id(c), T.case(c)) for c in T.CASES] + [("biased", T.biased_case())]
    for tag, (n, S, A, y, th, off, seed, nus, t_rep, t_obs) in every:
        m = P.margins(t_rep, t_obs)[:, P.compared(n)]
        print(tag, "%.3g" % m.min())
        assert np.isfinite(np.asarray(t_rep, dtype=np.float64)).all()
        assert m.min() > T.MARGIN_FLOOR, (tag, m.min())


def test_cases_cover_what_the_issue_names():
    ns, ks, Ss, nus = (set(c[j] for c in T.CASES) for j in range(4))
    assert ns == {3, 63, 64, 65, 129} and ks == {1, 16, 17} and Ss == {2, 64, 65, 130}
    assert nus == {1.5, 4.0, 50.0, T.CYCLE}
    seeds = set(c[4] for c in T.CASES)
    assert {0, 2 ** 64 - 1} <= seeds and any(s >> 32 and s != 2 ** 64 - 1 for s in seeds)
    assert any(c[5] for c in T.CASES)
    cyc = T.case_nu(T.CYCLE, 130)
    assert set(cyc[:64]) == set(T.NUS) and cyc[63] != cyc[64] and list(cyc[:4]) == [1.5, 4.0, 50.0, 1.5]


# ---- the surface ---------------------------------------------------------------------------------------
def test_nu_arguments_are_checked_before_anything_runs():
    A, y, th = P.make_case(5, 2, 6, 1)
    f = ppc.posterior_predictive_check
    with pytest.raises(ValueError, match="not both"):
        f(A, y, th, seed=1, nu=4.0, nu_draws=np.full(6, 4.0))
    for bad in (0.0, -1.0, float("inf"), float("nan"), "4", True):
        with pytest.raises(ValueError, match="nu must be None or a positive finite number"):
            f(A, y, th, seed=1, nu=bad)
    with pytest.raises(ValueError, match="shaped like the leading dimensions"):
        f(A, y, th, seed=1, nu_draws=np.full(5, 4.0))
    with pytest.raises(ValueError, match="shaped like the leading dimensions"):
        f(A, y, th.reshape(2, 3, 3), seed=1, nu_draws=np.full(6, 4.0))
    for bad in (0.0, -2.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="nu_draws must be positive and finite"):
            f(A, y, th, seed=1, nu_draws=np.r_[np.full(5, 4.0), bad])
    big = P.make_case(5, 2, 5000, 1)[2]
    with pytest.raises(ValueError, match="distinct values; at most 4096"):
        f(A, y, big, seed=1, nu_draws=np.linspace(1, 9, 5000))
    with pytest.raises(ValueError, match="seed must be"):
        f(A, y, th, seed=-1, nu=4.0)


class FakeContext:
    """Stands where _lib.default_context's context stands: records which entry point a call reaches
    and with what behind the seed."""

    def __init__(self):
        self.lock = threading.Lock()
        self.calls = []

    def _record(self, name, A, n, k, lda, layout, y, theta, n_draws, ldt, offset, seed, *noise):
        self.calls.append((name, int(n), int(n_draws), offset is not None, seed, noise))
        return {"t_rep": np.zeros((n_draws, 8)), "t_obs2": np.ones((n_draws, 2))}

    def ppc(self, *a):
        return self._record("ppc", *a)

    def ppc_t(self, *a):
        return self._record("ppc_t", *a)

    def ppc_tv(self, *a):
        return self._record("ppc_tv", *a)


def test_function_reaches_the_entry_point_of_its_likelihood(monkeypatch):
    fake = FakeContext()
    monkeypatch.setattr(_lib, "default_context", lambda device=0: fake)
    A, y, th = P.make_case(5, 2, 6, 1)
    g = ppc.posterior_predictive_check(A, y, th, seed=3)
    t = ppc.posterior_predictive_check(A, y, th, seed=3, nu=4)
    v = ppc.posterior_predictive_check(A, y, th.reshape(2, 3, 3), seed=3, burn=1,
                                       nu_draws=np.array([[9.0, 2.0, 4.0], [9.0, 4.0, 2.0]]))
    assert [c[0] for c in fake.calls] == ["ppc", "ppc_t", "ppc_tv"]
    assert fake.calls[0][4:] == (3, (0.0,)) and fake.calls[1][4:] == (3, (4.0,))
    name, n, S, has_off, seed, (values, index) = fake.calls[2]
    assert (n, S, has_off, seed) == (5, 4, False, 3)
    assert list(values) == [2.0, 4.0] and list(index) == [0, 1, 1, 0] and index.dtype == np.int32
    assert (g["likelihood"], g["nu_estimated"]) == ("gaussian", False)
    assert (t["likelihood"], t["nu_estimated"]) == ("student_t", False)
    assert (v["likelihood"], v["nu_estimated"]) == ("student_t", True) and v["n_draws"] == 4
    for out in (g, t, v):
        assert out["stats"] == ppc.PPC_STATS and out["seed"] == 3 and out["p_value"]["chi2"] == 0.0


def test_check_dispatch(monkeypatch):
    """check() checks the last fit under its own likelihood: the plain call for a Gaussian or a
    simplex fit, nu= after "student_t", nu_draws= after "nu": "estimate"; the old method keeps
    refusing a Student-t fit."""
    import pandas as pd
    from pybmc_amd.bmc import BayesianModelCombination
    df = pd.DataFrame({"N": [1, 2, 3], "Z": [1, 1, 2], "a": [1.0, 2.0, 3.0], "b": [1.5, 2.5, 2.0],
                       "truth": [1.2, 2.2, 2.6]})
    bmc = BayesianModelCombination(["a", "b"], {"p": df}, "truth")
    with pytest.raises(ValueError, match="train"):
        bmc.check()
    bmc.samples = np.abs(np.random.default_rng(0).standard_normal((6, 2))) + 0.1
    bmc.U_hat = np.ones((3, 1))
    bmc.Vt_hat = np.ones((1, 2))
    bmc.S_hat = np.ones(1)
    bmc.centered_experiment_train = np.array([0.1, -0.2, 0.3])
    bmc._predictions_mean_train = np.array([1.0, 2.0, 3.0])
    bmc.n_chains = 2
    fake = FakeContext()
    monkeypatch.setattr(_lib, "default_context", lambda device=0: fake)
    prior = [np.zeros(1), np.eye(1), 1.0, 0.02]

    for sampler in ("gibbs", "simplex"):
        bmc._trained_with = (sampler, prior)
        g = bmc.check(seed=11)
        old = bmc.posterior_predictive_check(seed=11)
        assert g["likelihood"] == "gaussian" and g["nu"] is None and g["nu_estimated"] is False
        assert all(np.array_equal(g[key], old[key]) for key in ("t_rep", "t_obs")) and g["p_value"] == old["p_value"]
    assert [c[0] for c in fake.calls] == ["ppc"] * 4 and all(c[1:5] == (3, 6, True, 11) for c in fake.calls)

    del fake.calls[:]
    bmc._trained_with = ("student_t", prior, 4.0)
    t = bmc.check(burn=1, seed=12)
    assert t["likelihood"] == "student_t" and t["nu"] == 4.0 and t["nu_estimated"] is False and t["n_draws"] == 4
    h = bmc.check(X=df[["a", "b", "truth"]], seed=13)
    assert h["nu"] == 4.0 and h["n_points"] == 3
    assert fake.calls == [("ppc_t", 3, 4, True, 12, (4.0,)), ("ppc_t", 3, 6, True, 13, (4.0,))]

    del fake.calls[:]
    bmc._trained_with = ("student_t", prior, "estimate")
    bmc.nu_samples = np.array([2.0, 3.0, 3.0, 8.0, 2.0, 3.0])
    e = bmc.check(burn=1, seed=14)
    assert e["likelihood"] == "student_t" and e["nu_estimated"] is True
    assert e["nu"] == pytest.approx(np.mean([3.0, 3.0, 2.0, 3.0]))
    name, n, S, has_off, seed, (values, index) = fake.calls[0]
    assert (name, n, S, has_off, seed) == ("ppc_tv", 3, 4, True, 14)
    assert list(values) == [2.0, 3.0] and list(index) == [1, 1, 0, 1]

    for call in (bmc.posterior_predictive_check, bmc.loo_predict):
        with pytest.raises(ValueError, match="supports the Gaussian Gibbs sampler only"):
            call()
    with pytest.raises(ValueError, match="DataFrame"):
        bmc.check(X=df.values)
    with pytest.raises(ValueError, match="truth"):
        bmc.check(X=df[["a", "b"]])


def test_header_keeps_abi_4_and_declares_the_entry_points():
    text = open(HEADER).read()
    assert re.search(r"#define\s+PYBMC_AMD_ABI_VERSION\s+4\b", text)
    assert _lib.ABI_VERSION == 4
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("bmc_ppc_t", "bmc_ppc_t_device", "bmc_ppc_tv", "bmc_ppc_tv_device"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.PROTOTYPES
    # the arguments of bmc_ppc without the dead `center`
    t = re.search(r"int\s+bmc_ppc_t\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    g = re.search(r"int\s+bmc_ppc\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    norm = lambda s: [" ".join(a.split()) for a in s.split(",")]
    assert [a for a in norm(g) if a != "double center"] == [a for a in norm(t) if a != "double nu"]
    assert "double nu" in norm(t) and "double center" not in norm(t)
    assert len(_lib.PROTOTYPES["bmc_ppc_tv"][1]) == len(_lib.PROTOTYPES["bmc_ppc"][1]) + 2


@pytest.mark.parametrize("n,S,k,want", [
    (3, 2, 1, (1, 1, 64, 64, 16)),
    (65, 130, 3, (2, 3, 128, 192, 16)),
    (200, 257, 33, (4, 5, 256, 320, 48)),
    (10000, 50000, 32, (157, 782, 10048, 50048, 32)),
])
def test_plan_is_unchanged_and_the_nu_rows_stand_beside_it(tmp_path, n, S, k, want):
    exe = tmp_path / "ppc_t_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, "ppc_t_plan_check.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), str(n), str(S), str(k), "256"], check=True, capture_output=True, text=True)
    p = dict((kv.split("=")[0], int(kv.split("=")[1])) for kv in r.stdout.split())
    assert p["ok"] == 1
    assert (p["point_tiles"], p["draw_tiles"], p["n_pad"], p["S_pad"], p["k_pad"]) == want
    n_pad, S_pad, k_pad = want[2:]
    assert p["bytes_Ap"] == n_pad * k_pad * 8 and p["bytes_yo"] == 2 * n_pad * 8
    assert p["bytes_Tp"] == S_pad * k_pad * 8 and p["bytes_sg"] == (3 * S_pad + k_pad + 16) * 8
    assert p["bytes_out"] == S * 10 * 8
    assert p["bytes_total"] == sum(p["bytes_" + key] for key in ("Ap", "yo", "Tp", "sg", "out"))
    assert p["bytes_nu"] == 2 * S_pad * 8 and p["max_nu_values"] == 4096
