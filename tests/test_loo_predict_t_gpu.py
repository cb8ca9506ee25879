"""The leave-one-out predictive moments under the Student-t likelihood on the MI355X
(kernels_loo.hip's t PREDICT passes: the append in two phases, the bucket, the fit;
pybmc_amd.scoring.psis_loo_predict(nu= / nu_draws=)) against the dense numpy reference of
tests/loo_predict_t_reference.py: every point, every output.

elpd_loo_i, pareto_k and lppd must be the bits of psis_loo under the same likelihood arguments (whose
own distance to its reference test_tscore_gpu.py and test_tscore_nu_gpu.py hold).  The bars of the
other outputs are 100 x the rounding floor of the float64 reference against np.longdouble, measured
on these very cases by test_loo_predict_t_host.py (the margin of test_loo_predict_gpu.py, for the
reasons its docstring gives); the floors are loo_predict_t_reference.FLOORS:

    loo_mean 9.4e-15 absolute   loo_sd 1.7e-13 absolute   loo_pit 4.6e-16 absolute   ess 1.7e-15 relative
    k > 1:   7.9e-15            4.6e-13           3.4e-16            3.8e-15

loo_sd is +inf exactly where the reference's is (some scored nu <= 2).  The device's distribution
function alone is held to mpmath within 64 x the error of scipy.special.stdtr on the same arguments,
the bar of the g++ build in test_loo_predict_t_host.py.  No point is left out.

Measured on the MI355X: see DESIGN.md 4.7.1."""
import numpy as np
import pytest

import loo_predict_reference as L
import loo_predict_t_host_build as HB
import loo_predict_t_reference as LT
import psis_reference as P
import score_reference as R
import tscore_reference as T

pytestmark = pytest.mark.gpu

TOL = {key: 100 * v for key, v in LT.FLOORS.items()}
TOL_BIG = {key: 100 * v for key, v in LT.FLOORS_BIG.items()}
WORST = {}          # (printed by the last test: the largest distance of each output over the file)


def distances(got, ref):
    """{key: [n] distance of the device to the reference}, in the units of the floors; loo_sd where
    the reference is +inf: 0 if the device's is too, else +inf."""
    out = {}
    for key in LT.NEW_KEYS:
        r = np.asarray(ref[key], dtype=np.float64)
        g = np.asarray(got[key], dtype=np.float64)
        with np.errstate(invalid="ignore"):
            d = np.abs(g - r)
            d = d / r if key == "ess" else d
        out[key] = np.where(np.isinf(r), np.where(g == r, 0.0, np.inf), d)
    return out


def check(got, ref, tag=""):
    """Every point of the case against the reference; prints the figures before it asserts."""
    big = np.asarray(ref["pareto_k"], dtype=np.float64) > 1
    d = distances(got, ref)
    print(f"{tag}: " + "  ".join(
        f"{key} {d[key][~big].max() if (~big).any() else 0:.3e} (k > 1: "
        f"{d[key][big].max() if big.any() else 0:.3e})" for key in LT.NEW_KEYS))
    for key in LT.NEW_KEYS:
        for cls, sel in (("", ~big), (" k>1", big)):
            if sel.any():
                WORST[key + cls] = max(WORST.get(key + cls, 0.0), float(d[key][sel].max()))
    for key in LT.NEW_KEYS:
        assert not np.isnan(got[key]).any(), (tag, key)
        assert np.all(d[key][~big] <= TOL[key]), (tag, key)
        assert np.all(d[key][big] <= TOL_BIG[key]), (tag, key)
    assert np.all(got["ess"] >= 1 - 1e-12) and np.all(got["loo_sd"] > 0), tag
    assert np.all((got["loo_pit"] >= 0) & (got["loo_pit"] <= 1)), tag
    assert np.isfinite(got["loo_mean"]).all() and np.isfinite(got["loo_pit"]).all(), tag


def raw(A, y, th, **kw):
    """The pointwise outputs under the reference's names, and the whole dict."""
    from pybmc_amd import psis_loo_predict
    out = psis_loo_predict(A, y, th, **kw)
    got = {"elpd_loo": out["elpd_loo_i"], "pareto_k": out["pareto_k"], "lppd": out["lppd"]}
    got.update({key: out[key] for key in LT.NEW_KEYS})
    return got, out


def same_bits_as_psis_loo(got, A, y, th, **lik):
    from pybmc_amd import psis_loo
    plain = psis_loo(A, y, th, **lik)
    for key, pk in (("elpd_loo", "elpd_loo_i"), ("pareto_k", "pareto_k"), ("lppd", "lppd")):
        assert np.array_equal(got[key], plain[pk], equal_nan=True), key


def run_group(name):
    for tag, (A, y, th), spec in LT.group(name):
        lik = LT.lik_of(spec, len(th))
        got, out = raw(A, y, th, **lik)
        check(got, LT.reference(tag, (A, y, th), spec), tag)
        same_bits_as_psis_loo(got, A, y, th, **lik)
        inf_sd = bool(np.any(LT.nu_of_draws(len(th), **lik) <= 2))
        assert np.isinf(got["loo_sd"]).all() if inf_sd else np.isfinite(got["loo_sd"]).all(), tag
    return out


# ---- parity -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu", LT.NUS)
def test_fixed_nu_on_the_cases_of_the_t_scores(nu):
    """tscore_reference's shape cases (k 1 .. 33, points across the 64-wide tile, S = 2 .. 4097), its
    40-unit outlier and its tiny residuals, at nu = 1.5 (loo_sd = +inf), 4 and 50."""
    run_group(f"tscore nu={nu:g}")


@pytest.mark.parametrize("spec", (LT.CYCLE_INF, LT.CYCLE_FINITE, 2.0, 2.5), ids=str)
def test_nu_per_draw_and_the_edge_of_the_variance(spec):
    """nu cycling over the draws through 1.5 / 4 / 50 (loo_sd = +inf everywhere) and through
    2.5 / 4 / 50 (finite); nu = 2 exactly (+inf) and 2.5 (finite: the variance term is 5 sigma^2)."""
    run_group(f"spec {spec}")


@pytest.mark.parametrize("k", (3, 33))
def test_shapes_on_both_sides_of_every_rule(k):
    """psis_reference.shape_cases: points across the 64-wide tile; draws below and at the M >= 5 rule
    (24, 25), lanes without a draw, several splits (4097: above the candidate cap, so the select and
    the bucket pass run); both layouts, lda and ldt wider than the rows.  k = 3 at nu = 4 through the
    _t entry point, k = 33 with nu cycling through 2.5 / 4 / 50 through the _tv one."""
    from pybmc_amd import _lib
    ctx = _lib.default_context(0)
    for (tag, (A, y, th), spec), (case, n, S, _) in zip(LT.group(f"shapes k={k}"), P.shape_cases(k)):
        assert A.shape == (n, k) and len(th) == S
        pad_a, pad_t = (case % 3) * 2, (case % 2) * 3
        if case % 2:
            buf = np.full((k, n + pad_a), np.nan)
            buf[:, :n] = A.T
            lda, layout = n + pad_a, _lib.BMC_COL_MAJOR
        else:
            buf = np.full((n, k + pad_a), np.nan)
            buf[:, :k] = A
            lda, layout = k + pad_a, _lib.BMC_ROW_MAJOR
        tb = np.full((S, k + 1 + pad_t), np.nan)
        tb[:, :k + 1] = th
        args = (buf, n, k, lda, layout, y, tb, S, k + 1 + pad_t)
        with ctx.lock:
            if isinstance(spec, tuple):
                values, index = np.unique(LT.cycling(S, spec), return_inverse=True)
                index = np.ascontiguousarray(index, dtype=np.int32)
                got = ctx.psis_loo_predict_tv(*args, values, index)
                plain = ctx.psis_loo_tv(*args, values, index)
            else:
                got = ctx.psis_loo_predict_t(*args, spec)
                plain = ctx.psis_loo_t(*args, spec)
        if S < 25:
            assert np.isinf(got["pareto_k"]).all()
        check(got, LT.reference(tag, (A, y, th), spec), f"{tag} layout={layout} lda={lda} ldt={k + 1 + pad_t}")
        for key in ("elpd_loo", "pareto_k", "lppd"):
            assert np.array_equal(got[key], plain[key]), (tag, key)


def test_a_run_of_ties_across_the_cutoff():
    """The S / 2 ties of test_loo_predict_gpu.py under nu = 4 (4500 ties against a cap of 1024: the
    bucket is one repeated value, its payload comes from the t bucket pass and the tie rule shares
    the weights).  The same draws permuted: the values alone decide."""
    (tag, (A, y, th), spec), = LT.group("ties")
    ref = LT.reference(tag, (A, y, th), spec)
    got, _ = raw(A, y, th, nu=spec)
    check(got, ref, tag)
    same_bits_as_psis_loo(got, A, y, th, nu=spec)
    got_p, _ = raw(A, y, th[np.random.default_rng(3).permutation(len(th))], nu=spec)
    check(got_p, ref, tag + ", permuted")
    M = P.tail_length(len(th))
    ll = LT.loglik(A, y, th, nu=spec)
    assert sum(np.sort(row)[M] == np.sort(row)[M - 1] for row in ll) >= 20


def test_mirror_draws_tie_with_opposite_residuals():
    """Every ll[0, s] occurs twice with opposite r (the t density is even in r): shared weights give
    loo_mean[0] = 0 and loo_pit[0] = 1/2 to the rounding level, F(z) + F(-z) being 1 to the last bit."""
    for tag, (A, y, th), spec in LT.group("mirror"):
        lik = LT.lik_of(spec, len(th))
        got, _ = raw(A, y, th, **lik)
        check(got, LT.reference(tag, (A, y, th), spec), tag)
        print(tag, "loo_mean[0]", got["loo_mean"][0], "loo_pit[0] - 1/2", got["loo_pit"][0] - 0.5)
        assert abs(got["loo_mean"][0]) <= TOL["loo_mean"]
        assert abs(got["loo_pit"][0] - 0.5) <= TOL["loo_pit"]


# ---- bit equalities ---------------------------------------------------------------------------------
def test_bit_equalities():
    """One value in nu_draws gives the bits of nu=; host arrays and device tensors, two calls and a
    Fortran-ordered A give the same bits; elpd_loo_i, pareto_k and lppd are psis_loo's."""
    import torch
    A, y, th = R.random_case(300, 7, 5000, 21)
    chains = th.reshape(2, 2500, 8)
    for lik, single in (({"nu": 4.0}, {"nu_draws": np.full((2, 2500), 4.0)}),
                        ({"nu": 1.5}, {"nu_draws": np.full((2, 2500), 1.5)})):
        a, _ = raw(A, y, chains, **lik)
        b, _ = raw(A, y, chains, **lik)
        c, _ = raw(A, y, torch.as_tensor(chains, device="cuda:0"), **lik)
        d, _ = raw(np.asfortranarray(A), y, chains, **lik)
        e, _ = raw(A, y, chains, **single)
        f, _ = raw(A, y, torch.as_tensor(chains, device="cuda:0"), **single)
        for key in a:
            for other in (b, c, d, e, f):
                assert np.array_equal(a[key], other[key]), (lik, key)
        same_bits_as_psis_loo(a, A, y, chains, **lik)
    nd = LT.cycling(5000, LT.CYCLE_FINITE).reshape(2, 2500)
    g, _ = raw(A, y, chains, nu_draws=nd, burn=100, thin=3)
    h, _ = raw(A, y, torch.as_tensor(chains, device="cuda:0"), nu_draws=nd, burn=100, thin=3)
    for key in g:
        assert np.array_equal(g[key], h[key]), key
    same_bits_as_psis_loo(g, A, y, chains, nu_draws=nd, burn=100, thin=3)
    check(g, LT.pointwise(A, y, R.pool(chains, 100, 3), nu_draws=R.pool(nd[..., None], 100, 3)[:, 0]),
          "burn and thin, nu per draw")


# ---- the device's distribution function alone ---------------------------------------------------------
def test_the_device_cdf_alone():
    """Two identical draws (the fewest the call accepts): equal ll, so nothing is smoothed, the weights
    are equal and loo_pit_i = F_nu(y_i / sigma) with a_i . beta = 0.  |z| from 1e-20 to 1e6 in both
    signs and 0, at every nu of the host grid, against mpmath; the bar is the host test's, 64 x the
    largest error of scipy.special.stdtr on the same arguments."""
    import mpmath as mp
    from scipy.special import stdtr
    mag = np.concatenate([10.0 ** np.linspace(-20, 6, 53), LT.CDF_SPECIAL[1:], [0.7, 1.3, 2.0, 5.0, 9.0]])
    z = np.concatenate([[0.0], mag, -mag])
    sigma = 0.5                                       # (a power of two: y / sigma is exact)
    A = np.zeros((len(z), 2))
    A[:, 0] = 1.0
    th = np.array([[0.0, 0.0, sigma]] * 2)
    y = z * sigma
    zz = y / sigma                                    # (what the device divides)
    for nu in LT.CDF_NUS:
        got, _ = raw(A, y, th, nu=nu)
        assert np.isinf(got["pareto_k"]).all()
        with mp.workdps(40):
            want = []
            for v in zz:
                tail = mp.betainc(mp.mpf(nu) / 2, mp.mpf(1) / 2, 0, mp.mpf(nu) / (mp.mpf(nu) + mp.mpf(float(v)) ** 2),
                                  regularized=True) / 2
                want.append(tail if v < 0 else 1 - tail)
            err = max(float(abs(mp.mpf(float(g)) - w)) for g, w in zip(got["loo_pit"], want))
            floor = max(float(abs(mp.mpf(float(g)) - w)) for g, w in zip(stdtr(nu, zz), want))
        host = HB.t_cdf(zz, nu)[0]
        differ = int(np.count_nonzero(host != got["loo_pit"]))
        worst = float(np.abs(host - got["loo_pit"]).max())
        print(f"nu={nu}: device {err:.3e}  stdtr {floor:.3e}  ratio {err / floor:.1f}; {differ} of "
              f"{len(zz)} differ from the g++ build, by {worst:.2e} at most")
        assert err <= 64 * floor
        assert got["loo_pit"][0] == 0.5
        np.testing.assert_allclose(got["loo_mean"], 0.0, atol=0)
        assert np.all(got["ess"] == 2.0)


# ---- point flags, refusals ------------------------------------------------------------------------------
def test_a_nan_point_is_nan_and_its_neighbours_are_untouched():
    A, y, th = T.shape_case(5, 65, 513)
    for lik in ({"nu": 4.0}, {"nu": 1.5}, {"nu_draws": LT.cycling(513, LT.CYCLE_FINITE)}):
        base, _ = raw(A, y, th, **lik)
        A2 = A.copy()
        A2[17, 2] = np.nan
        got, _ = raw(A2, y, th, **lik)
        ok = np.arange(65) != 17
        for key in LT.KEYS:
            assert np.isnan(got[key][17]), (lik, key)
            assert np.array_equal(got[key][ok], base[key][ok]), (lik, key)
        y2 = y.copy()
        y2[64] = np.inf
        got, _ = raw(A, y2, th, **lik)
        for key in LT.NEW_KEYS:
            assert np.isnan(got[key][64]) and np.array_equal(got[key][:64], base[key][:64]), (lik, key)


def test_c_abi_refuses_nu_outside_the_range():
    from pybmc_amd import _lib
    ctx = _lib.default_context(0)
    A, y, th = R.random_case(10, 3, 20, 1)
    args = (A, 10, 3, 3, 0, y, th, 20, 4)
    idx = np.zeros(20, dtype=np.int32)
    for nu in (0.05, 1000.5):
        with pytest.raises(ValueError, match="between 0.06 and 1000"):
            ctx.psis_loo_predict_t(*args, nu)
        with pytest.raises(ValueError, match="between 0.06 and 1000"):
            ctx.psis_loo_predict_tv(*args, np.array([4.0, nu]), idx)
    with pytest.raises(ValueError, match="nu must be positive"):
        ctx.psis_loo_predict_t(*args, 0.0)
    with pytest.raises(ValueError, match="n_draws"):
        ctx.psis_loo_predict_t(A, 10, 3, 3, 0, y, th, 1, 4, 4.0)
    with pytest.raises(ValueError, match="1863225"):
        ctx.psis_loo_predict_t_device(1, 10, 3, 3, 0, 1, 1, 1863226, 4, 4.0)
    out = ctx.psis_loo_predict_t(*args, 4.0)        # the context is still usable
    assert np.isfinite(out["loo_pit"]).all()


# ---- end to end -----------------------------------------------------------------------------------------
def test_loo_predictions_of_a_t_fit_of_the_planted_problem():
    """The planted 200 x 3 problem of the robust tests (robust_cases.planted("200x3")), 4 chains of
    200 + 1800 sweeps as there: the rows the t fit down-weights stand out in the leave-one-out
    residuals and sit in the tails of their predictive distributions."""
    import pandas as pd
    import robust_cases as RC
    from pybmc_amd import BayesianModelCombination
    y, X, prior, _, idx = RC.planted("200x3")
    df = pd.DataFrame({"a": [0.0], "b": [0.0], "c": [0.0], "d": [0.0], "truth": [0.0]})
    b = BayesianModelCombination(["a", "b", "c", "d"], {"p": df}, truth_column_name="truth")
    b.U_hat = X
    b.S_hat = np.sqrt(np.diag(prior[1]))
    b.Vt_hat = np.zeros((3, 4))
    b.centered_experiment_train = y
    b._predictions_mean_train = np.zeros(len(y))
    b.train({"sampler": "student_t", "nu": 4, "n_chains": 4, "iterations": RC.PLANTED_BURN + RC.PLANTED_KEEP,
             "seeds": [41, 42, 43, 44]})
    out = b.loo_predictions(burn=RC.PLANTED_BURN)
    assert out["likelihood"] == "student_t" and out["nu"] == 4.0 and out["n_draws"] == 4 * RC.PLANTED_KEEP
    for key in ("loo_mean", "loo_sd", "loo_pit", "ess", "elpd_loo_i", "predicted", "residual"):
        assert out[key].shape == (len(y),) and np.isfinite(out[key]).all(), key
    clean = np.setdiff1d(np.arange(len(y)), idx)
    res, dev = np.abs(out["residual"]), np.abs(2 * out["loo_pit"] - 1)
    print(f"planted |residual| min {res[idx].min():.3f}, clean median {np.median(res[clean]):.3f}; planted "
          f"|2 pit - 1| min {dev[idx].min():.5f}, clean median {np.median(dev[clean]):.3f}; loo_rmse "
          f"{out['loo_rmse']:.4f}")
    assert res[idx].min() > np.median(res[clean])
    assert dev[idx].min() > 0.99          # (8 to 16 sigma out under t_4: a tail of 1e-3 or less)
    with pytest.raises(ValueError, match="supports the Gaussian Gibbs sampler only"):
        b.loo_predict()
    chains = np.asarray(b.samples).reshape(4, -1, 4)
    ref = LT.pointwise(X, y, R.pool(chains, RC.PLANTED_BURN), nu=4.0)
    got = {"elpd_loo": out["elpd_loo_i"], "pareto_k": out["pareto_k"], "lppd": out["lppd"]}
    got.update({key: out[key] for key in LT.NEW_KEYS})
    check(got, ref, "planted 200 x 3")


def test_print_the_largest_distances_of_this_file():
    """Not a check of its own: the largest distance per output over every case above, next to the
    bars (what DESIGN.md 4.7.1 records)."""
    for key in sorted(WORST):
        base = key.split()[0]
        print(f"{key}: {WORST[key]:.3e}  (bar {(TOL_BIG if 'k>1' in key else TOL)[base]:.1e})")
