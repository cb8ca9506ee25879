"""Power-scaling sensitivity on the GPU (-m gpu): kernels_sens.hip through the C ABI and the Python
API against the long-double numpy reference (tests/sens_reference.py).

Bars.  Each is about 16 x the larger of (a) the largest deviation of the GPU from the long-double
reference over PARITY_CASES, measured on an MI355X, and (b) the float64 reference's own deviation
from it, rounded up to a power of ten (the measured pairs are in MEASURED below).
Log densities and the weighted mean and sd are compared relative to their scale, the weights
relative to the mean weight 1 / S, pareto_k, cjs and psens absolutely.  The bars of the weights and
of cjs are many orders below what could move a case of test_sensitivity_reference.py across the
0.05 threshold (those lie a factor 2 away)."""
import os
import re

import numpy as np
import pytest

import sens_reference as SR
from conftest import ROOT, load_golden
from pybmc_amd import gibbs_sampler, power_scale_sensitivity, power_scale_weights, sensitivity_summary

pytestmark = pytest.mark.gpu

LD = np.longdouble

# quantity: (GPU vs long double, float64 reference vs long double), the maxima over PARITY_CASES
MEASURED = {
    "logdens": (2.8e-15, 3.2e-15),
    "weights": (6.1e-14, 4.5e-14),
    "pareto_k": (1.1e-13, 1.4e-13),
    "mean": (1.1e-15, 1.7e-15),
    "sd": (9.2e-13, 5.8e-15),     # about the column's median: digits go where the weights move the mean far
    "cjs": (6.2e-16, 1.3e-15),
    "psens": (5.0e-15, 1.9e-14),
}
BARS = {"logdens": 1e-13, "weights": 1e-12, "pareto_k": 1e-11, "mean": 1e-13, "sd": 1e-10, "cjs": 1e-13,
        "psens": 1e-12}


def _constant(header, name):
    text = open(os.path.join(ROOT, "pybmc_amd", "csrc", header)).read()
    return int(re.search(name + r" = (\d+);", text).group(1))


CHUNK = _constant("bmc_sens_plan.h", "SENS_CHUNK")
TILE = _constant("bmc_rank_plan.h", "RANK_BLOCK") * _constant("bmc_rank_plan.h", "RANK_ITEMS")
GRID = (0.5, 0.8, 1.25, 2.0)

# name: (N, k, S or (C, T, burn, thin), n_models, dense C0, grid of alphas, components)
DEFAULT = ("prior", "likelihood")
PARITY_CASES = {
    "S24_no_fit": (7, 3, 24, 0, True, None, DEFAULT),
    "S25_first_fit": (7, 3, 25, 2, True, None, DEFAULT),
    "S225_rules_cross": (7, 1, 225, 0, True, None, DEFAULT),
    "S226_rules_cross": (7, 1, 226, 2, True, None, DEFAULT),
    "chunk_minus_1": (7, 1, CHUNK - 1, 0, False, None, DEFAULT),
    "chunk": (7, 3, CHUNK, 0, True, None, DEFAULT),
    "chunk_plus_1": (7, 1, CHUNK + 1, 2, True, None, DEFAULT),
    "tile_minus_1": (7, 3, TILE - 1, 2, True, None, DEFAULT),
    "tile": (7, 1, TILE, 0, True, None, DEFAULT),
    "tile_plus_1": (7, 3, TILE + 1, 0, False, None, DEFAULT),
    "chains_odd_kept": (629, 3, (3, 1367, 1, 2), 4, True, None, DEFAULT),
    "k32": (629, 32, 700, 0, True, None, DEFAULT),
    "k32_weights": (7, 32, 301, 5, True, None, DEFAULT),
    "grid": (629, 3, 1000, 2, True, GRID, DEFAULT),
    "all_components": (29, 3, 500, 2, True, (0.8, 1.25), SR.COMPONENTS),
}


def _make(name):
    N, k, S, n_models, dense, grid, comps = PARITY_CASES[name]
    seed = 7000 + sorted(PARITY_CASES).index(name)
    kw = {}
    if isinstance(S, tuple):
        C, T, burn, thin = S
        A, y, theta, prior, Vt = SR.random_case(N, k, C * T, seed, n_models, dense)
        samples = theta.reshape(C, T, k + 1)
        pooled = samples[:, burn::thin].reshape(-1, k + 1)
        assert (pooled.shape[0] // C) % 2 == 1          # an odd kept length: no draw may be dropped
        kw = {"burn": burn, "thin": thin}
    else:
        A, y, theta, prior, Vt = SR.random_case(N, k, S, seed, n_models, dense)
        samples = pooled = theta
    return A, y, samples, pooled, prior, Vt, grid, comps, kw


_REF = {}


def reference(name):
    """The long-double and the float64 reference of a case, computed once."""
    if name not in _REF:
        A, y, _, pooled, prior, Vt, grid, comps, _ = _make(name)
        alphas = (0.99, 1.01) + tuple(grid or ())
        _REF[name] = tuple(SR.sensitivity(A, y, pooled, prior, Vt, alphas, comps, dtype=dt)
                           for dt in (LD, np.float64))
    return _REF[name]


def _scaled(ref):
    """The reference's arrays and the scale each deviation is taken against."""
    S = ref["lp"].shape[1]
    lb, ls, ll = ref["lp"]
    logdens = np.stack([lb + ls, ll, lb, ls])
    scale_col = (np.abs(ref["mean"]) + ref["sd"])
    return {"logdens": (logdens, np.maximum(1, np.abs(logdens))),
            "weights": (ref["weights"], LD(1) / S),
            "pareto_k": (ref["pareto_k"], None),
            "mean": (ref["mean"], scale_col), "sd": (ref["sd"], scale_col),
            "cjs": (ref["cjs"], None),
            "psens": (SR.psens(ref["cjs"][:, 0], ref["cjs"][:, 1]), None)}


def _dev(got, want, scale):
    got, want = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    assert got.shape == want.shape, (got.shape, want.shape)
    both_inf = np.isinf(got) & np.isinf(want) & (np.sign(got) == np.sign(want))
    with np.errstate(invalid="ignore"):
        d = np.where(both_inf, 0, np.abs(got - want))
    if scale is not None:
        d = d / scale
    assert not np.isnan(d).any()
    return float(d.max()) if d.size else 0.0


def gpu_arrays(res, weights):
    """A result of power_scale_sensitivity in the reference's layout."""
    comps = res["components"]
    return {"logdens": np.stack([res["log_prior"], res["log_lik"], res["log_prior_beta"],
                                 res["log_prior_sigma2"]]),
            "weights": weights,
            "pareto_k": np.stack([res["pareto_k"][c] for c in comps]),
            "mean": np.stack([res["mean"][c] for c in comps]),
            "sd": np.stack([res["sd"][c] for c in comps]),
            "cjs": np.stack([res["cjs"][c] for c in comps]),
            "psens": np.stack([res["psens"][c] for c in comps])}


def deviations(name):
    """{quantity: (GPU vs long double, float64 reference vs long double)} of one parity case."""
    A, y, samples, pooled, prior, Vt, grid, comps, kw = _make(name)
    res = power_scale_sensitivity(A, y, samples, prior, Vt, alphas=grid, components=comps, **kw)
    assert res["n_draws"] == pooled.shape[0] and tuple(res["components"]) == tuple(comps)
    alphas = res["alphas"]
    w = np.stack([[power_scale_weights(A, y, samples, prior, component=c, alpha=a, **kw)[0]
                   for a in alphas[:2]] for c in comps])
    ld, f64 = reference(name)
    want, got = _scaled(ld), gpu_arrays(res, w)
    host = _scaled(f64)
    out = {}
    for key, (ref, scale) in want.items():
        g, h = got[key], host[key][0]
        if key == "weights":
            ref, h = ref[:, :2], h[:, :2]
        out[key] = (_dev(g, ref, scale), _dev(h, ref, scale))
    return out


@pytest.mark.parametrize("name", sorted(PARITY_CASES))
def test_parity_with_the_long_double_reference(name):
    dev = deviations(name)
    for key, (gpu, f64) in dev.items():
        print(f"{name} {key}: gpu {gpu:.3e}  float64 reference {f64:.3e}  bar {BARS[key]:.0e}")
    for key, (gpu, _) in dev.items():
        assert gpu <= BARS[key], (name, key, gpu)
    ld, _ = reference(name)
    M = min(ld["lp"].shape[1] // 5, int(np.ceil(3 * np.sqrt(ld["lp"].shape[1]))))
    assert np.all(np.isinf(ld["pareto_k"])) == (M < 5)


# ---- ties -------------------------------------------------------------------------------------------
def _tied_case():
    """A chain with long runs of repeated rows, as Metropolis makes them, a constant quantity
    column, and runs long enough to straddle the tail's cutoff."""
    rng = np.random.default_rng(77)
    A, y, theta, prior, _ = SR.random_case(40, 2, 260, 78, 0)
    runs = rng.integers(1, 40, size=260)
    theta = np.repeat(theta, runs, axis=0)[:3001]
    Vt = np.array([[0.5, 0.0], [-0.25, 0.0]])        # the second model weight is the constant 1/2
    return A, y, np.ascontiguousarray(theta), prior, Vt


def test_ties_agree_with_the_reference_and_a_constant_column_is_exactly_zero():
    A, y, theta, prior, Vt = _tied_case()
    S = theta.shape[0]
    M = min(S // 5, int(np.ceil(3 * np.sqrt(S))))
    assert len(np.unique(theta[:, 0])) < S // 5 and M >= 5
    res = power_scale_sensitivity(A, y, theta, prior, Vt, alphas=(0.5, 2.0))
    ref = SR.sensitivity(A, y, theta, prior, Vt, (0.99, 1.01, 0.5, 2.0), dtype=LD)
    w = np.stack([[power_scale_weights(A, y, theta, prior, component=c, alpha=a)[0] for a in (0.99, 1.01)]
                  for c in ("prior", "likelihood")])
    want, got = _scaled(ref), gpu_arrays(res, w)
    for key, (r, scale) in want.items():
        d = _dev(got[key], r[:, :2] if key == "weights" else r, scale)
        print(f"ties {key}: {d:.3e}")
        assert d <= BARS[key], key
    assert np.all(got["cjs"][:, :, -1] == 0.0) and np.all(got["psens"][:, -1] == 0.0)
    assert np.all(got["sd"][:, :, -1] == 0.0) and np.all(got["mean"][:, :, -1] == 0.5)
    # the draws in another order: the same estimate, to rounding
    perm = np.random.default_rng(5).permutation(S)
    res_p = power_scale_sensitivity(A, y, np.ascontiguousarray(theta[perm]), prior, Vt, alphas=(0.5, 2.0))
    got_p = gpu_arrays(res_p, w)
    for key in ("pareto_k", "mean", "sd", "cjs", "psens"):
        scale = want[key][1]
        assert _dev(got_p[key], got[key], scale) <= 2 * BARS[key], key
    assert _dev(got_p["logdens"][:, np.argsort(perm)], got["logdens"], want["logdens"][1]) == 0.0


# ---- bits -------------------------------------------------------------------------------------------
NUMERIC = ("log_prior", "log_lik", "log_prior_beta", "log_prior_sigma2")


def same_bits(a, b, alphas_a=None, alphas_b=None):
    ok = all(np.array_equal(a[key], b[key], equal_nan=True) for key in NUMERIC)
    ia = range(len(a["alphas"])) if alphas_a is None else alphas_a
    ib = range(len(b["alphas"])) if alphas_b is None else alphas_b
    for c in a["components"]:
        ok = ok and np.array_equal(a["psens"][c], b["psens"][c], equal_nan=True)
        for key in ("mean", "sd", "cjs", "pareto_k"):
            ok = ok and np.array_equal(a[key][c][list(ia)], b[key][c][list(ib)], equal_nan=True)
    return ok


def test_bits_do_not_depend_on_the_call_the_grid_the_batch_or_where_the_arrays_live():
    import torch
    A, y, samples, pooled, prior, Vt, _, comps, kw = _make("chains_odd_kept")
    a = power_scale_sensitivity(A, y, samples, prior, Vt, alphas=GRID, **kw)
    assert same_bits(a, power_scale_sensitivity(A, y, samples, prior, Vt, alphas=GRID, **kw))
    # an alpha alone and the same alpha inside a grid
    one = power_scale_sensitivity(A, y, samples, prior, Vt, alphas=[GRID[2]], **kw)
    assert same_bits(one, a, [0, 1, 2], [0, 1, 2 + 2])
    # one column per batch, three per batch, and the default
    for cpb in (1, 3):
        assert same_bits(a, power_scale_sensitivity(A, y, samples, prior, Vt, alphas=GRID,
                                                    cols_per_batch=cpb, **kw))
    # device tensors
    d = power_scale_sensitivity(A, y, torch.as_tensor(samples, device="cuda"), prior, Vt, alphas=GRID, **kw)
    assert same_bits(a, d)
    # pooled by hand: burn and thin are the caller's slicing
    assert same_bits(a, power_scale_sensitivity(A, y, pooled, prior, Vt, alphas=GRID))
    wa = power_scale_weights(A, y, samples, prior, component="likelihood", alpha=GRID[0], **kw)
    wb = power_scale_weights(A, y, torch.as_tensor(samples, device="cuda"), prior, component="likelihood",
                             alpha=GRID[0], **kw)
    assert np.array_equal(wa[0], wb[0]) and wa[1] == wb[1] == a["pareto_k"]["likelihood"][2]
    assert abs(wa[0].sum() - 1) < 1e-12


# ---- non-finite input ----------------------------------------------------------------------------------
def test_non_finite_input_is_nan_where_defined_and_nothing_else():
    A, y, theta, prior, Vt = SR.random_case(20, 2, 2100, 31, n_models=2)
    good = power_scale_sensitivity(A, y, theta, prior, Vt, components=SR.COMPONENTS)
    assert not any(good["component_flags"].values()) and not good["column_flags"].any()
    # NaN in one coefficient: its column, the model weights built from it, and every component
    bad = theta.copy()
    bad[7, 1] = np.nan
    r = power_scale_sensitivity(A, y, bad, prior, Vt, components=SR.COMPONENTS)
    assert all(r["component_flags"].values())
    assert list(r["column_flags"]) == [False, True, False, True, True]
    for c in SR.COMPONENTS:
        assert np.isnan(r["psens"][c]).all() and np.isnan(r["pareto_k"][c]).all()
        assert np.isnan(r["cjs"][c]).all() and np.isnan(r["mean"][c]).all()
    assert np.isnan(r["log_prior"][7]) and np.isnan(r["log_lik"][7])
    assert np.isfinite(np.delete(r["log_lik"], 7)).all()
    assert set(r["diagnosis"]) == {"-"}
    w, k = power_scale_weights(A, y, bad, prior)
    assert np.isnan(w).all() and np.isnan(k)
    # NaN in an input of one model weight alone: that column alone
    Vb = Vt.copy()
    Vb[0, 1] = np.nan
    r = power_scale_sensitivity(A, y, theta, prior, Vb, components=SR.COMPONENTS)
    assert not any(r["component_flags"].values())
    assert list(r["column_flags"]) == [False, False, False, False, True]
    for c in SR.COMPONENTS:
        assert np.isnan(r["cjs"][c][:, 4]).all() and np.isnan(r["psens"][c][4])
        assert np.array_equal(r["cjs"][c][:, :4], good["cjs"][c][:, :4])
        assert np.array_equal(r["pareto_k"][c], good["pareto_k"][c])
    # a draw with sigma <= 0 (zero, negative), an infinite coefficient, a NaN in A or y
    for s_bad in (0.0, -0.3):
        bad = theta.copy()
        bad[2000, 2] = s_bad
        r = power_scale_sensitivity(A, y, bad, prior, Vt, components=SR.COMPONENTS)
        assert all(r["component_flags"].values())
        assert all(np.isnan(r["psens"][c]).all() for c in SR.COMPONENTS)
    bad = theta.copy()
    bad[0, 0] = np.inf
    assert all(power_scale_sensitivity(A, y, bad, prior, Vt)["component_flags"].values())
    for what in ("A", "y"):
        Ab, yb = A.copy(), y.copy()
        if what == "A":
            Ab[3, 1] = np.nan
        else:
            yb[19] = np.inf
        r = power_scale_sensitivity(Ab, yb, theta, prior, Vt, components=SR.COMPONENTS)
        assert r["component_flags"] == {"prior": False, "likelihood": True, "prior_beta": False,
                                        "prior_sigma2": False}
        assert np.isnan(r["psens"]["likelihood"]).all()
        assert np.array_equal(r["psens"]["prior"], good["psens"]["prior"])


# ---- the diagnosis, end to end -------------------------------------------------------------------------
def test_a_conflicting_tight_prior_is_diagnosed_as_prior_data_conflict():
    A, y, prior = SR.conflict_problem()
    chains = gibbs_sampler(y, A, 3000, prior, n_chains=2, seeds=[11, 12])
    res = power_scale_sensitivity(A, y, chains, prior, burn=500)
    ref = SR.sensitivity(A, y, chains[:, 500:].reshape(-1, 2), prior, dtype=LD)
    for ci, c in enumerate(("prior", "likelihood")):
        want = SR.psens(ref["cjs"][ci, 0], ref["cjs"][ci, 1])
        print(c, res["psens"][c], want, res["pareto_k"][c])
        assert _dev(res["psens"][c], want, None) <= BARS["psens"]
        assert want[0] >= 2 * SR.THRESHOLD                # the reference is clear of the threshold
    assert res["diagnosis"][0] == "prior-data conflict"
    t = sensitivity_summary(res)
    assert t.loc["beta_0", "diagnosis"] == "prior-data conflict" and list(t.index) == ["beta_0", "sigma"]


def test_the_reference_defaults_on_its_own_problem_show_nothing():
    g = load_golden("gibbs_ortho629x3")
    prior = [g["b0"], g["C0"], float(g["nu0"]), float(g["s20"])]
    chains = gibbs_sampler(g["y"], g["X"], 2500, prior, n_chains=2, seeds=[21, 22])
    res = power_scale_sensitivity(g["X"], g["y"], chains, prior, g["Vt"], burn=500)
    ref = SR.sensitivity(g["X"], g["y"], chains[:, 500:].reshape(-1, 4), prior, g["Vt"], dtype=LD)
    want = SR.psens(ref["cjs"][0, 0], ref["cjs"][0, 1])
    print(res["psens"], want)
    assert _dev(res["psens"]["prior"], want, None) <= BARS["psens"]
    assert want.max() <= SR.THRESHOLD / 2
    assert set(res["diagnosis"]) == {"-"} and len(res["diagnosis"]) == 3 + 1 + g["Vt"].shape[1]


def test_bmc_prior_sensitivity():
    import score_reference as R
    from pybmc_amd import BayesianModelCombination
    train, models = R.three_component_frame(400, seed=1)
    b = BayesianModelCombination(models, {"p": train}, truth_column_name="truth")
    b.orthogonalize("p", train, components_kept=3, method="svd")
    b.train({"iterations": 1500, "burn": 300, "n_chains": 2, "seeds": [1, 2]})
    s = np.asarray(b.samples).reshape(2, -1, 4)
    yc = np.asarray(b.centered_experiment_train, dtype=np.float64)
    prior = [np.zeros(3), np.diag(b.S_hat ** 2), 1.0, 0.02]
    a = b.prior_sensitivity(burn=100, alphas=[0.9])
    w = power_scale_sensitivity(b.U_hat, yc, s, prior, b.Vt_hat, burn=100, alphas=[0.9])
    assert same_bits(a, w) and a["columns"] == ["beta_0", "beta_1", "beta_2", "sigma"] + models
    assert a["n_draws"] == 2 * (s.shape[1] - 100)
    tight = b.prior_sensitivity(training_options={"b_mean_cov": np.diag(b.S_hat ** 2) * 1e-4})
    assert not same_bits(tight, b.prior_sensitivity())
    b.train({"iterations": 300, "burn": 100, "sampler": "simplex"})
    with pytest.raises(ValueError, match="simplex"):
        b.prior_sensitivity()


# ---- argument errors ----------------------------------------------------------------------------------
def test_argument_errors():
    A, y, theta, prior, Vt = SR.random_case(12, 2, 40, 1, n_models=2)
    for kwargs in ({"alphas": [1.0]}, {"alphas": [0.0]}, {"alphas": [-0.5]}, {"alphas": np.linspace(1.1, 2, 65)},
                   {"components": ("posterior",)}):
        with pytest.raises(ValueError):
            power_scale_sensitivity(A, y, theta, prior, Vt, **kwargs)
    with pytest.raises(ValueError):
        power_scale_sensitivity(A, y[:-1], theta, prior, Vt)
    with pytest.raises(ValueError):
        power_scale_sensitivity(A, y, theta, [prior[0][:1], prior[1], 1.0, 0.02], Vt)
    # a grid of 64 is allowed; C0 must be positive definite (the sampler's singular error)
    r = power_scale_sensitivity(A, y, theta, prior, Vt, alphas=np.linspace(1.1, 2, 64))
    assert r["cjs"]["prior"].shape == (66, 5)
    with pytest.raises(np.linalg.LinAlgError, match="Singular matrix"):
        power_scale_sensitivity(A, y, theta, [prior[0], np.array([[1.0, 2.0], [2.0, 1.0]]), 1.0, 0.02], Vt)
    from pybmc_amd import _lib
    ctx = _lib.default_context(0)
    args = (A, 12, 2, 2, 0, y, theta, 40, 3, prior, None)
    with pytest.raises(ValueError, match="alpha"):
        ctx.power_sensitivity(*args, [1.0], 3)
    with pytest.raises(ValueError, match="components"):
        ctx.power_sensitivity(*args, [1.01], 0)
    with pytest.raises(ValueError, match="ldt"):
        ctx.power_sensitivity(A, 12, 2, 2, 0, y, theta, 40, 2, prior, None, [1.01], 3)
    with pytest.raises(ValueError, match="n_draws"):
        ctx.power_sensitivity(A, 12, 2, 2, 0, y, theta, 1, 3, prior, None, [1.01], 3)
