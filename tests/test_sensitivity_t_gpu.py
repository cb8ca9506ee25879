"""Power-scaling sensitivity of Student-t fits on the GPU (-m gpu): sens_tsum_tile_kernel and
sens_logdens_t_kernel of kernels_sens.hip through the C ABI and the Python API against the
long-double numpy reference (tests/sens_t_reference.py), in the frame of tests/test_sensitivity_gpu.py.

Bars.  Per case and quantity the floor is the deviation of the float64 numpy reference from the
long-double one, computed here (no code under test in it); the bar is the larger of that quantity's
bar in test_sensitivity_gpu.BARS and 64 x the floor (the convention of DESIGN.md 4.9).  MEASURED holds
the largest GPU deviation and the largest floor over PARITY_CASES on an MI355X."""
import numpy as np
import pytest

import sens_reference as SR
import sens_t_reference as ST
import tscore_reference as TS
from pybmc_amd import (T_COMPONENTS, gibbs_sampler, gibbs_sampler_robust, power_scale_sensitivity,
                       power_scale_weights, sensitivity_summary)
from test_sensitivity_gpu import BARS, CHUNK, GRID, _dev, same_bits

pytestmark = pytest.mark.gpu

LD = np.longdouble
BAR_FACTOR = 64

# quantity: (GPU vs long double, float64 reference vs long double), the maxima over PARITY_CASES
MEASURED = {
    "logdens": (2.0e-15, 2.4e-15),
    "weights": (2.9e-15, 2.2e-15),
    "pareto_k": (8.5e-14, 7.9e-14),
    "mean": (1.3e-16, 3.2e-16),
    "sd": (2.2e-16, 2.1e-16),
    "cjs": (1.1e-16, 1.7e-15),
    "psens": (3.8e-15, 6.0e-14),
}

DEFAULT = ("prior", "likelihood")
CYCLE = "cycle"
NU_GRID = np.array([1.5, 2.5, 4.0, 7.0, 12.0, 25.0, 50.0])
NU_WEIGHT = np.array([1.0, 3.0, 5.0, 4.0, 3.0, 2.0, 1.0])

# name: (N, k, S or (C, T, burn, thin), n_models, nu or CYCLE, grid of alphas, components, what is special)
PARITY_CASES = {
    "N7_S25_k3_first_fit": (7, 3, 25, 2, 4.0, None, DEFAULT, None),
    "N64_S63_k1": (64, 1, 63, 0, 1.5, None, DEFAULT, None),
    "N65_S64_k16": (65, 16, 64, 0, 50.0, None, DEFAULT, None),
    "N129_S65_k17": (129, 17, 65, 2, 4.0, None, DEFAULT, None),
    "S129_k32": (7, 32, 129, 0, 1.5, None, DEFAULT, None),
    "chunk_minus_1": (7, 1, CHUNK - 1, 0, 50.0, None, DEFAULT, None),
    "chunk_plus_1": (7, 3, CHUNK + 1, 2, 4.0, None, DEFAULT, None),
    "outlier": (65, 3, 129, 0, 4.0, None, DEFAULT, "outlier"),
    "tiny_residuals": (65, 3, 65, 0, 4.0, None, DEFAULT, "tiny"),
    "chains_odd_kept": (629, 3, (3, 1367, 1, 2), 4, 4.0, None, DEFAULT, None),
    "cycle": (7, 1, 65, 0, CYCLE, None, DEFAULT + ("prior_nu",), None),
    "cycle_weights": (65, 3, 129, 2, CYCLE, None, DEFAULT + ("prior_nu",), None),
    "all_components": (29, 3, 500, 2, CYCLE, (0.8, 1.25), T_COMPONENTS, None),
}


def _make(name):
    """The arrays of a case: what the library is given (`samples`, `lik`, `kw`) and what the
    reference is (`pooled`, `nu`: a number or (values, index, log prior))."""
    N, k, S, n_models, nu, grid, comps, special = PARITY_CASES[name]
    seed = 9000 + sorted(PARITY_CASES).index(name)
    kw = {}
    total = S[0] * S[1] if isinstance(S, tuple) else S
    A, y, theta, prior, Vt = SR.random_case(N, k, total, seed, n_models, True)
    if special == "outlier":
        y = y.copy()
        y[0] += 40.0
    if special == "tiny":     # residuals 1e-20 .. 1e-1: tscore_reference.tiny_case, every coefficient 0
        A, y, theta = TS.tiny_case()
        prior = [np.zeros(k), np.eye(k), 1.0, 0.02]
    draws = NU_GRID[np.arange(total) % 7] if nu == CYCLE else None
    if isinstance(S, tuple):
        C, T, burn, thin = S
        samples = theta.reshape(C, T, k + 1)
        pooled = samples[:, burn::thin].reshape(-1, k + 1)
        assert (pooled.shape[0] // C) % 2 == 1
        kw = {"burn": burn, "thin": thin}
        if draws is not None:
            draws = draws.reshape(C, T)
        pooled_draws = None if draws is None else draws[:, burn::thin].reshape(-1)
    else:
        samples = pooled = theta
        pooled_draws = draws
    if nu == CYCLE:
        values, index = ST.nu_table(pooled_draws)
        ref_nu = lambda dt: (values, index, ST.log_prior_of(values, NU_GRID, NU_WEIGHT, dt))
        lik = {"nu_draws": draws, "nu_grid": NU_GRID, "nu_prior": NU_WEIGHT}
    else:
        ref_nu = lambda dt: nu
        lik = {"nu": nu}
    return {"A": A, "y": y, "samples": samples, "pooled": pooled, "prior": prior, "Vt": Vt, "grid": grid,
            "comps": comps, "kw": kw, "lik": lik, "ref_nu": ref_nu}


_REF = {}


def reference(name):
    """The long-double and the float64 reference of a case, computed once."""
    if name not in _REF:
        c = _make(name)
        alphas = (0.99, 1.01) + tuple(c["grid"] or ())
        _REF[name] = tuple(ST.sensitivity(c["A"], c["y"], c["pooled"], c["prior"], c["ref_nu"](dt), c["Vt"],
                                          alphas, c["comps"], dtype=dt) for dt in (LD, np.float64))
    return _REF[name]


def _scaled(ref):
    """The reference's arrays and the scale each deviation is taken against (test_sensitivity_gpu's,
    with the fifth log density; a column that is the constant 0 has no scale: absolute)."""
    S = ref["lp"].shape[1]
    lb, ls, ll, ln = ref["lp"]
    logdens = np.stack([lb + ls + ln, ll, lb, ls, ln])
    scale_col = np.abs(ref["mean"]) + ref["sd"]
    scale_col = np.where(scale_col == 0, 1, scale_col)
    return {"logdens": (logdens, np.maximum(1, np.abs(logdens))),
            "weights": (ref["weights"], LD(1) / S),
            "pareto_k": (ref["pareto_k"], None),
            "mean": (ref["mean"], scale_col), "sd": (ref["sd"], scale_col),
            "cjs": (ref["cjs"], None),
            "psens": (SR.psens(ref["cjs"][:, 0], ref["cjs"][:, 1]), None)}


def gpu_arrays(res, weights):
    """A result of power_scale_sensitivity in the reference's layout."""
    comps = res["components"]
    return {"logdens": np.stack([res["log_prior"], res["log_lik"], res["log_prior_beta"],
                                 res["log_prior_sigma2"], res["log_prior_nu"]]),
            "weights": weights,
            "pareto_k": np.stack([res["pareto_k"][c] for c in comps]),
            "mean": np.stack([res["mean"][c] for c in comps]),
            "sd": np.stack([res["sd"][c] for c in comps]),
            "cjs": np.stack([res["cjs"][c] for c in comps]),
            "psens": np.stack([res["psens"][c] for c in comps])}


def deviations(name):
    """{quantity: (GPU vs long double, float64 reference vs long double)} of one parity case."""
    c = _make(name)
    args = (c["A"], c["y"], c["samples"], c["prior"])
    res = power_scale_sensitivity(*args, c["Vt"], alphas=c["grid"], components=c["comps"], **c["kw"], **c["lik"])
    assert res["n_draws"] == c["pooled"].shape[0] and tuple(res["components"]) == tuple(c["comps"])
    assert res["likelihood"] == "student_t"
    assert (res["columns"][-1] == "nu") == ("nu_draws" in c["lik"])
    w = np.stack([[power_scale_weights(*args, component=comp, alpha=a, **c["kw"], **c["lik"])[0]
                   for a in res["alphas"][:2]] for comp in c["comps"]])
    ld, f64 = reference(name)
    want, got, host = _scaled(ld), gpu_arrays(res, w), _scaled(f64)
    out = {}
    for key, (ref, scale) in want.items():
        g, h = got[key], host[key][0]
        if key == "weights":
            ref, h = ref[:, :2], h[:, :2]
        out[key] = (_dev(g, ref, scale), _dev(h, ref, scale))
    return out


def bar(key, floor):
    return max(BARS[key], BAR_FACTOR * floor)


@pytest.mark.parametrize("name", sorted(PARITY_CASES))
def test_parity_with_the_long_double_reference(name):
    dev = deviations(name)
    for key, (gpu, f64) in dev.items():
        print(f"{name} {key}: gpu {gpu:.3e}  floor {f64:.3e}  bar {bar(key, f64):.1e}")
    for key, (gpu, f64) in dev.items():
        assert gpu <= bar(key, f64), (name, key, gpu, f64)
    ld, _ = reference(name)
    M = min(ld["lp"].shape[1] // 5, int(np.ceil(3 * np.sqrt(ld["lp"].shape[1]))))
    # (a component of few distinct values, prior_nu, may have a tail of one value: nothing smoothed)
    assert np.all(np.isinf(ld["pareto_k"][:2])) == (M < 5)


def test_cases_cover_what_the_issue_names():
    c = list(PARITY_CASES.values())
    assert {7, 64, 65, 129, 629} <= {v[0] for v in c} and {1, 3, 16, 17, 32} <= {v[1] for v in c}
    assert {25, 63, 64, 65, 129, CHUNK - 1, CHUNK + 1, (3, 1367, 1, 2)} <= {v[2] for v in c}
    assert {1.5, 4.0, 50.0, CYCLE} <= {v[4] for v in c} and {"outlier", "tiny"} <= {v[7] for v in c}
    assert {bool(v[3]) for v in c if v[4] == CYCLE} == {True, False}
    assert PARITY_CASES["all_components"][6] == T_COMPONENTS and len(T_COMPONENTS) == 5
    assert PARITY_CASES["chains_odd_kept"][0] == 629
    tiny = _make("tiny_residuals")
    r = np.abs(tiny["y"][:, None] - tiny["A"] @ tiny["pooled"][:, :3].T)
    assert r.min() == 1e-20 and r.max() <= 0.1
    assert _make("outlier")["y"][0] > 30


# ---- bits ---------------------------------------------------------------------------------------------
def _numeric(a, b, cols=slice(None)):
    ok = all(np.array_equal(a[key], b[key], equal_nan=True)
             for key in ("log_prior", "log_lik", "log_prior_beta", "log_prior_sigma2", "log_prior_nu"))
    for c in a["components"]:
        ok = ok and np.array_equal(a["psens"][c][cols], b["psens"][c][cols], equal_nan=True)
        ok = ok and np.array_equal(a["pareto_k"][c], b["pareto_k"][c], equal_nan=True)
        for key in ("mean", "sd", "cjs"):
            ok = ok and np.array_equal(a[key][c][:, cols], b[key][c][:, cols], equal_nan=True)
    return ok


def test_one_distinct_nu_draw_gives_the_bits_of_the_fixed_nu_call():
    c = _make("chains_odd_kept")
    args = (c["A"], c["y"], c["samples"], c["prior"], c["Vt"])
    Q = 3 + 1 + 4
    fixed = power_scale_sensitivity(*args, alphas=GRID, components=SR.COMPONENTS, nu=4.0, **c["kw"])
    table = power_scale_sensitivity(*args, alphas=GRID, components=SR.COMPONENTS,
                                    nu_draws=np.full(c["samples"].shape[:2], 4.0), **c["kw"])
    assert table["columns"] == fixed["columns"] + ["nu"] and len(fixed["columns"]) == Q
    assert _numeric(table, fixed, slice(0, Q)) and np.all(fixed["log_prior_nu"] == 0)
    for comp in SR.COMPONENTS:      # the nu column is a constant
        assert np.all(table["cjs"][comp][:, Q] == 0) and np.all(table["mean"][comp][:, Q] == 4.0)
    # with a prior of nu on one value: lp_nu = log 1 = 0, still the same bits
    prior = power_scale_sensitivity(*args, alphas=GRID, components=SR.COMPONENTS,
                                    nu_draws=np.full(c["samples"].shape[:2], 4.0), nu_grid=[4.0], nu_prior=[2.0],
                                    **c["kw"])
    assert _numeric(prior, table)
    wf = power_scale_weights(*args[:4], component="likelihood", alpha=GRID[0], nu=4.0, **c["kw"])
    wt = power_scale_weights(*args[:4], component="likelihood", alpha=GRID[0],
                             nu_draws=np.full(c["samples"].shape[:2], 4.0), **c["kw"])
    assert np.array_equal(wf[0], wt[0]) and wf[1] == wt[1] == fixed["pareto_k"]["likelihood"][2]


def test_bits_do_not_depend_on_the_call_the_grid_the_batch_or_where_the_arrays_live():
    import torch
    for name, comps in (("chains_odd_kept", DEFAULT), ("cycle_weights", T_COMPONENTS)):
        c = _make(name)
        args, kw = (c["A"], c["y"], c["samples"], c["prior"], c["Vt"]), {**c["kw"], **c["lik"], "components": comps}
        a = power_scale_sensitivity(*args, alphas=GRID, **kw)
        assert same_bits(a, power_scale_sensitivity(*args, alphas=GRID, **kw))
        one = power_scale_sensitivity(*args, alphas=[GRID[2]], **kw)
        assert same_bits(one, a, [0, 1, 2], [0, 1, 2 + 2])
        for cpb in ((1, 3) if name == "cycle_weights" else (3,)):   # (the nu column alone in a batch, too)
            assert same_bits(a, power_scale_sensitivity(*args, alphas=GRID, cols_per_batch=cpb, **kw))
        dev = (args[0], args[1], torch.as_tensor(c["samples"], device="cuda"), args[3], args[4])
        d = power_scale_sensitivity(*dev, alphas=GRID, **kw)
        assert same_bits(a, d) and np.array_equal(a["log_prior_nu"], d["log_prior_nu"])
        wa = power_scale_weights(*args[:4], component="likelihood", alpha=GRID[0], **c["kw"], **c["lik"])
        wb = power_scale_weights(*dev[:4], component="likelihood", alpha=GRID[0], **c["kw"], **c["lik"])
        assert np.array_equal(wa[0], wb[0]) and wa[1] == wb[1] == a["pareto_k"]["likelihood"][2]
        assert abs(wa[0].sum() - 1) < 1e-12


def test_the_priors_are_the_gaussian_calls_and_the_gaussian_call_is_undisturbed():
    c = _make("cycle_weights")
    args = (c["A"], c["y"], c["samples"], c["prior"], c["Vt"])
    before = power_scale_sensitivity(*args, alphas=GRID, components=SR.COMPONENTS)
    t = power_scale_sensitivity(*args, alphas=GRID, components=SR.COMPONENTS, nu=4.0)
    v = power_scale_sensitivity(*args, alphas=GRID, components=T_COMPONENTS, **c["lik"])
    after = power_scale_sensitivity(*args, alphas=GRID, components=SR.COMPONENTS)
    for r in (t, v):
        for key in ("log_prior_beta", "log_prior_sigma2"):
            assert np.array_equal(r[key], before[key])
        for comp in ("prior_beta", "prior_sigma2"):      # and so everything made of them alone
            for key in ("mean", "sd", "cjs", "pareto_k"):
                cols = slice(0, len(before["columns"]))
                got = r[key][comp] if key == "pareto_k" else r[key][comp][:, cols]
                assert np.array_equal(got, before[key][comp])
        assert not np.array_equal(r["log_lik"], before["log_lik"])
    assert np.array_equal(t["log_prior"], before["log_prior"])          # no prior of nu: lp_nu = 0
    assert same_bits(before, after) and after["likelihood"] == "gaussian" and after["log_prior_nu"] is None
    assert np.array_equal(before["column_flags"], after["column_flags"])


# ---- non-finite input ----------------------------------------------------------------------------------
def test_non_finite_input_is_nan_where_defined_and_nothing_else():
    A, y, theta, prior, Vt = SR.random_case(20, 2, 2100, 31, n_models=2)
    draws = NU_GRID[np.arange(2100) % 7]
    lik = {"nu_draws": draws, "nu_grid": NU_GRID, "nu_prior": NU_WEIGHT}
    good = power_scale_sensitivity(A, y, theta, prior, Vt, components=T_COMPONENTS, **lik)
    assert not any(good["component_flags"].values()) and not good["column_flags"].any()
    logs = ("log_prior", "log_lik", "log_prior_beta", "log_prior_sigma2", "log_prior_nu")
    for row, col, value, cols in ((7, 1, np.nan, [False, True, False, True, True, False]),
                                  (2000, 2, 0.0, None), (2000, 2, -0.3, None), (2000, 2, np.inf, None),
                                  (0, 0, np.inf, None)):
        bad = theta.copy()
        bad[row, col] = value
        for kw in (lik, {"nu": 4.0}):
            comps = T_COMPONENTS if kw is lik else SR.COMPONENTS
            r = power_scale_sensitivity(A, y, bad, prior, Vt, components=comps, **kw)
            assert all(r["component_flags"].values())
            for c in comps:
                assert np.isnan(r["psens"][c]).all() and np.isnan(r["pareto_k"][c]).all()
                assert np.isnan(r["cjs"][c]).all() and np.isnan(r["mean"][c]).all()
            for key in logs:
                assert np.isnan(r[key][row]) and np.isfinite(np.delete(r[key], row)).all(), (key, value)
            if cols is not None:
                assert list(r["column_flags"]) == cols[:len(r["columns"])]
            if kw is lik:       # every other draw has the bits of the clean call
                for key in logs:
                    assert np.array_equal(np.delete(r[key], row), np.delete(good[key], row))
        w, kh = power_scale_weights(A, y, bad, prior, component="prior_nu", **lik)
        assert np.isnan(w).all() and np.isnan(kh)
    # an infinity in A or y poisons the likelihood only
    for what in ("A", "y"):
        Ab, yb = A.copy(), y.copy()
        if what == "A":
            Ab[3, 1] = np.inf
        else:
            yb[19] = -np.inf
        r = power_scale_sensitivity(Ab, yb, theta, prior, Vt, components=T_COMPONENTS, **lik)
        assert r["component_flags"] == {"prior": False, "likelihood": True, "prior_beta": False,
                                        "prior_sigma2": False, "prior_nu": False}
        assert np.isnan(r["psens"]["likelihood"]).all() and np.isnan(r["log_lik"]).all()
        for c in ("prior", "prior_beta", "prior_sigma2", "prior_nu"):
            assert np.array_equal(r["psens"][c], good["psens"][c])
            assert np.array_equal(r["pareto_k"][c], good["pareto_k"][c])
        assert not r["column_flags"].any()


def test_a_bad_table_is_an_error_and_the_context_stays_usable():
    import torch
    from pybmc_amd import _lib
    A, y, theta, prior, Vt = SR.random_case(12, 2, 40, 1, n_models=2)
    ctx = _lib.default_context(0)
    args = (A, 12, 2, 2, 0, y, theta, 40, 3, prior, None, [0.99, 1.01])
    index = (np.arange(40) % 2).astype(np.int32)
    lp = np.log([0.25, 0.75])
    with ctx.lock:
        good = ctx.power_sensitivity_tv(*args, 31, 0, False, [2.0, 5.0], index, lp)
        for values in ([2.0, 0.0], [2.0, -1.0], [np.nan, 5.0], [2.0, np.inf]):
            with pytest.raises(ValueError, match="nu_values"):
                ctx.power_sensitivity_tv(*args, 3, 0, False, values, index, None)
        for nu in (0.0, -2.0, np.nan, np.inf):
            with pytest.raises(ValueError, match="nu must be positive and finite"):
                ctx.power_sensitivity_t(*args, 3, 0, False, nu)
        for bad_lp in ([0.0, np.nan], [-np.inf, 0.0]):
            with pytest.raises(ValueError, match="nu_log_prior"):
                ctx.power_sensitivity_tv(*args, 3, 0, False, [2.0, 5.0], index, bad_lp)
        with pytest.raises(ValueError, match="prior_nu"):      # bit 4 without a prior
            ctx.power_sensitivity_tv(*args, 16, 0, False, [2.0, 5.0], index, None)
        with pytest.raises(ValueError, match="prior_nu"):
            ctx.power_sensitivity_t(*args, 16, 0, False, 4.0)
        with pytest.raises(ValueError, match="components"):
            ctx.power_sensitivity_tv(*args, 32, 0, False, [2.0, 5.0], index, lp)
        for off in (-1, 2):                                       # a host index, before any launch
            bad = index.copy()
            bad[17] = off
            with pytest.raises(ValueError, match="nu_index must index nu_values"):
                ctx.power_sensitivity_tv(*args, 3, 0, False, [2.0, 5.0], bad, None)
        # a device index: clamped where it is read, reported after the run
        dA, dy, dth = (torch.as_tensor(v, device="cuda") for v in (A, y, theta))
        dargs = (dA.data_ptr(), 12, 2, 2, 0, dy.data_ptr(), dth.data_ptr(), 40, 3, prior, None, [0.99, 1.01])
        for off in (-1, 2):
            bad = index.copy()
            bad[17] = off
            d_bad = torch.as_tensor(bad, device="cuda")
            torch.cuda.synchronize()
            with pytest.raises(ValueError, match="nu_index must index nu_values"):
                ctx.power_sensitivity_tv_device(*dargs, 3, 0, False, [2.0, 5.0], d_bad.data_ptr(), None)
        d_index = torch.as_tensor(index, device="cuda")
        torch.cuda.synchronize()
        on_device = ctx.power_sensitivity_tv_device(*dargs, 31, 0, False, [2.0, 5.0], d_index.data_ptr(), lp)
        again = ctx.power_sensitivity_tv(*args, 31, 0, False, [2.0, 5.0], index, lp)
    for r in (on_device, again):                                  # the next call is correct
        for key in ("logdens", "pareto_k", "mean", "sd", "cjs"):
            assert np.array_equal(r[key], good[key]) and np.isfinite(r[key][np.isfinite(good[key])]).all()
    ref = ST.sensitivity(A, y, theta, prior, ([2.0, 5.0], index, lp), None, (0.99, 1.01), T_COMPONENTS, dtype=LD)
    assert good["logdens"].shape == (4, 40) and good["cjs"].shape == (5, 2, 4)
    assert _dev(good["cjs"], ref["cjs"], None) <= BARS["cjs"]
    assert _dev(good["logdens"], ref["lp"], np.maximum(1, np.abs(ref["lp"]))) <= BARS["logdens"]


# ---- the readings, end to end ---------------------------------------------------------------------------
def _psens_against_reference(res, ref, comps):
    """The device's psens against the long-double reference's on the same draws, within the bar
    (the floor is not computed here: the existing bar alone, the tighter of the two)."""
    want = {}
    for ci, c in enumerate(comps):
        want[c] = SR.psens(ref["cjs"][ci, 0], ref["cjs"][ci, 1])
        print(c, res["psens"][c], want[c], res["pareto_k"][c])
        assert _dev(res["psens"][c], want[c], None) <= BARS["psens"], c
    return want


def test_a_conflicting_tight_prior_is_diagnosed_under_the_t_likelihood():
    """Reading (a).  The reference sampler of tests/robust_reference.py on this problem (2 chains of
    3000 sweeps, 500 dropped, numpy variates) gives psens of beta_0: prior 0.41, likelihood 0.52;
    the threshold is 0.05."""
    A, y, prior = SR.conflict_problem()
    chains = gibbs_sampler_robust(y, A, 3000, prior, 4.0, n_chains=2, seeds=[11, 12])
    res = power_scale_sensitivity(A, y, chains, prior, burn=500, nu=4.0)
    ref = ST.sensitivity(A, y, chains[:, 500:].reshape(-1, 2), prior, 4.0, dtype=LD)
    want = _psens_against_reference(res, ref, DEFAULT)
    assert want["prior"][0] >= 2 * SR.THRESHOLD and want["likelihood"][0] >= 2 * SR.THRESHOLD
    assert res["diagnosis"][0] == "prior-data conflict"
    t = sensitivity_summary(res)
    assert t.loc["beta_0", "diagnosis"] == "prior-data conflict" and list(t.index) == ["beta_0", "sigma"]


def nu_prior_problem(N=200, seed=5, noise=0.5):
    """Gaussian noise under a prior that holds nu near 2: (A, y, prior, nu prior weights on the
    default grid: the Gamma(20, rate 10) density times nu_g)."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((N, 2))
    y = A @ np.array([1.0, -0.5]) + noise * rng.standard_normal(N)
    grid = np.geomspace(1.0, 100.0, 64)
    return A, y, [np.zeros(2), 10.0 * np.eye(2), 1.0, 0.02], grid, grid * (grid ** 19 * np.exp(-10.0 * grid))


def test_the_posterior_of_nu_restates_a_tight_prior_and_the_coefficients_do_not():
    """Reading (b).  With the default prior of nu the reference sampler of
    tests/robust_nu_reference.py (2 chains of 3000 sweeps, 500 dropped) gives psens[prior_nu] of the
    nu column 0.029 at N = 40 and 0.031, 0.035, 0.038, 0.039 at N = 30, 20, 12, 8: the value of a
    posterior that IS that prior, below the threshold at any N.  So the prior is made tight instead
    (Gamma(20, 10) on the default grid: nu near 2, which Gaussian noise contradicts) and N = 200:
    the reference's psens[prior_nu] is then 0.187 for nu, 0.014 and 0.010 for the coefficients
    (0.106, 0.0095, 0.0087 at N = 100; 0.073, 0.0063, 0.0058 at N = 40)."""
    A, y, prior, grid, weight = nu_prior_problem()
    chains, nu = gibbs_sampler_robust(y, A, 3000, prior, "estimate", n_chains=2, seeds=[21, 22],
                                      nu_prior=weight, return_nu=True)
    comps = ("prior", "likelihood", "prior_nu")
    res = power_scale_sensitivity(A, y, chains, prior, burn=500, nu_draws=nu, nu_prior=weight, components=comps)
    assert res["columns"] == ["beta_0", "beta_1", "sigma", "nu"]
    values, index = ST.nu_table(nu[:, 500:].reshape(-1))
    ref = ST.sensitivity(A, y, chains[:, 500:].reshape(-1, 3), prior,
                         (values, index, ST.log_prior_of(values, grid, weight, LD)), None, (0.99, 1.01), comps,
                         dtype=LD)
    want = _psens_against_reference(res, ref, comps)
    assert want["prior_nu"][3] >= 2 * SR.THRESHOLD and want["prior_nu"][:2].max() <= SR.THRESHOLD / 2
    assert res["psens"]["prior_nu"][3] >= SR.THRESHOLD and np.all(res["psens"]["prior_nu"][:2] < SR.THRESHOLD)
    t = sensitivity_summary(res)
    assert list(t.columns) == list(comps) + ["diagnosis"] and t.loc["nu", "prior_nu"] >= SR.THRESHOLD


# ---- BayesianModelCombination.sensitivity -----------------------------------------------------------------
def test_bmc_sensitivity_reads_each_kind_of_fit_under_its_own_likelihood():
    import score_reference as R
    from pybmc_amd import BayesianModelCombination
    train, models = R.three_component_frame(400, seed=1)
    b = BayesianModelCombination(models, {"p": train}, truth_column_name="truth")
    b.orthogonalize("p", train, components_kept=3, method="svd")
    yc = np.asarray(b.centered_experiment_train, dtype=np.float64)
    prior = [np.zeros(3), np.diag(b.S_hat ** 2), 1.0, 0.02]
    names = ["beta_0", "beta_1", "beta_2", "sigma"] + models

    b.train({"iterations": 1500, "burn": 300, "n_chains": 2, "seeds": [1, 2]})
    g = b.sensitivity(burn=100, alphas=[0.9])
    assert same_bits(g, b.prior_sensitivity(burn=100, alphas=[0.9])) and g["likelihood"] == "gaussian"
    assert g["columns"] == names

    b.train({"iterations": 1200, "burn": 300, "n_chains": 2, "seeds": [1, 2], "sampler": "student_t", "nu": 5.0})
    s = np.asarray(b.samples).reshape(2, -1, 4)
    t = b.sensitivity(burn=100, alphas=[0.9])
    w = power_scale_sensitivity(b.U_hat, yc, s, prior, b.Vt_hat, burn=100, alphas=[0.9], nu=5.0)
    assert same_bits(t, w) and t["columns"] == names and (t["likelihood"], t["nu"]) == ("student_t", 5.0)
    assert t["n_draws"] == 2 * (s.shape[1] - 100)
    with pytest.raises(ValueError, match="Gaussian Gibbs sampler only"):
        b.prior_sensitivity()

    b.train({"iterations": 1200, "burn": 300, "n_chains": 2, "seeds": [1, 2], "sampler": "student_t",
             "nu": "estimate"})
    s = np.asarray(b.samples).reshape(2, -1, 4)
    nu = np.asarray(b.nu_samples).reshape(2, -1)
    e = b.sensitivity(burn=100, alphas=[0.9])
    grid = np.geomspace(1.0, 100.0, 64)
    w = power_scale_sensitivity(b.U_hat, yc, s, prior, b.Vt_hat, burn=100, alphas=[0.9], nu_draws=nu,
                                nu_grid=grid, nu_prior=grid * (grid * np.exp(-0.1 * grid)),
                                components=("prior", "likelihood", "prior_nu"), models=models)
    assert same_bits(e, w) and e["columns"] == names + ["nu"] == w["columns"]
    assert e["components"] == ("prior", "likelihood", "prior_nu") and np.array_equal(e["log_prior_nu"], w["log_prior_nu"])
    assert e["nu"] == pytest.approx(nu[:, 100:].mean())
    b.train({"iterations": 300, "burn": 100, "sampler": "simplex"})
    with pytest.raises(ValueError, match="simplex"):
        b.sensitivity()
