"""Exact K-fold cross-validation under the Student-t likelihood on the device (-m gpu):
pybmc_amd.cv.kfold_cv(nu=...) and BayesianModelCombination.validate.

Bars (none taken from the code under test):
  chains   bit for bit (numpy.array_equal) against one gibbs_sampler_robust call per (fold, chain)
           on the training subset under the same seed, and likewise the row weights on the training
           rows: the folded kernel runs the unfolded kernel's code on the subset's own rows, start
           value, gamma shape and nu table;
  scores   elpd_cv_i against pointwise_log_likelihood(nu= / nu_draws=) on the held-out rows and the
           fold's draws: 1e-11 max(1, |ref|); cv_mean_i against A @ mean(draws): 1e-12 relative to
           the largest |mean| -- the bars of test_cv_gpu.py;
  repeats, memory orders, batches, burn / thin: bit for bit."""
import os

import numpy as np
import pytest

import robust_cases as RC
from pybmc_amd import compare_elpd, cv, gibbs_sampler_robust, pointwise_log_likelihood
from pybmc_amd._lib import BmcError

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
T = 40
TOL_ELPD, TOL_MEAN = 1e-11, 1e-12
GRID7 = np.array([1.0, 2.0, 3.0, 5.0, 8.0, 15.0, 40.0])
PRIOR7 = np.array([1.0, 2.0, 3.0, 3.0, 2.0, 1.0, 0.5])


def sizes_to_folds(sizes, seed):
    """Labels with exactly these fold sizes, shuffled: training rows of a fold are not contiguous."""
    labels = np.repeat(np.arange(len(sizes)), sizes)
    return np.random.default_rng(seed).permutation(labels).astype(np.int64)


def problem(n, k, seed):
    """A dense design with correlated columns; a tenth of the rows moved by several sigma."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, k)) + 0.3 * rng.standard_normal((n, 1))
    beta = rng.standard_normal(k)
    y = X @ beta + 0.2 * rng.standard_normal(n)
    bad = rng.choice(n, size=max(1, n // 10), replace=False)
    y[bad] += rng.choice([-1.0, 1.0], size=bad.size) * rng.uniform(1.5, 4.0, size=bad.size)
    return X, y, [np.zeros(k), 4.0 * np.eye(k), 1.0, 0.02]


# name -> (n, k, fold sizes, chains, nu): empty slabs and an n_train that is no multiple of 4
# (n_train 22 / 18 / 6); one case per kernel width (k = 3, 5, 9 at n about 70, k = 17 at n = 150: two
# column tiles); n_train = 64 (a multiple of 16), 65 (one more) and 33
CASES = {
    "empty_slabs": (23, 2, (1, 5, 17), 2, 4.0),
    "k3": (70, 3, (17, 18, 17, 18), 2, 1.5),
    "k5": (71, 5, (18, 18, 18, 17), 2, 50.0),
    "k9": (69, 9, (17, 17, 17, 18), 2, 4.0),
    "k17": (150, 17, (50, 49, 51), 2, 1.5),
    "mult16": (81, 2, (17, 16, 48), 2, 50.0),
}
_runs = {}


def run(name):
    """One kfold_cv call per case, shared by the tests and left unchanged."""
    if name not in _runs:
        n, k, sizes, C, nu = CASES[name]
        A, y, prior = problem(n, k, 100 + len(name) + k)
        folds = sizes_to_folds(sizes, k)
        out = cv.kfold_cv(A, y, prior, folds, T, n_chains=C, seed=5, nu=nu, return_draws=True,
                          return_row_weights=True)
        _runs[name] = (A, y, prior, folds, len(sizes), C, nu, out)
    return _runs[name]


def run_estimate():
    if "estimate" not in _runs:
        A, y, prior = problem(60, 3, 77)
        folds = sizes_to_folds((10, 20, 30), 3)
        out = cv.kfold_cv(A, y, prior, folds, T, n_chains=2, seed=6, nu="estimate", nu_grid=GRID7,
                          nu_prior=PRIOR7, nu_init=5.0, return_draws=True, return_row_weights=True)
        _runs["estimate"] = (A, y, prior, folds, 3, 2, out)
    return _runs["estimate"]


def solo(A, y, prior, folds, f, seed, nu, iters=T, **kw):
    tr = folds != f
    return gibbs_sampler_robust(y[tr], np.ascontiguousarray(A[tr]), iters, prior, nu, seeds=[seed],
                                return_row_weights=True, **kw)


@pytest.mark.parametrize("name", list(CASES))
def test_chains_are_the_subsets_chains_bit_for_bit(name):
    A, y, prior, folds, F, C, nu, out = run(name)
    n, k = A.shape
    assert out["draws"].shape == (F, C, T, k + 1) and out["row_weights"].shape == (F, C, n)
    assert out["likelihood"] == "student_t" and out["nu"] == nu and np.isfinite(out["draws"]).all()
    assert sorted(n - np.bincount(folds)) == sorted(n - np.array(CASES[name][2]))
    for f in range(F):
        tr = folds != f
        for c in range(C):
            ref, w = solo(A, y, prior, folds, f, out["seeds"][f, c], nu)
            assert np.array_equal(out["draws"][f, c], ref), (name, f, c)
            assert np.array_equal(out["row_weights"][f, c][tr], w), (name, f, c)
            assert np.isnan(out["row_weights"][f, c][~tr]).all()


def test_nu_estimated_bit_for_bit():
    """Folds of 10 / 20 / 30 rows: n_train 50 / 40 / 30, so the grid's constants c_g differ from fold
    to fold and one table for all folds would draw other indices."""
    A, y, prior, folds, F, C, out = run_estimate()
    assert out["nu_draws"].shape == (F, C, T) and np.isin(out["nu_draws"], GRID7).all()
    assert out["nu"] == pytest.approx(out["nu_draws"].mean(), rel=1e-14)
    assert len(np.unique(out["nu_draws"])) > 1
    for f in range(F):
        tr = folds != f
        for c in range(C):
            ref, w, nus = solo(A, y, prior, folds, f, out["seeds"][f, c], "estimate", nu_grid=GRID7,
                               nu_prior=PRIOR7, nu_init=5.0, return_nu=True)
            assert np.array_equal(out["draws"][f, c], ref), (f, c)
            assert np.array_equal(out["nu_draws"][f, c], nus), (f, c)
            assert np.array_equal(out["row_weights"][f, c][tr], w), (f, c)


def score_errors(A, y, folds, F, out, **lik):
    worst_e = worst_m = 0.0
    for f in range(F):
        held = folds == f
        Ah, yh = np.ascontiguousarray(A[held]), y[held]
        like = {key: (v[f] if key == "nu_draws" else v) for key, v in lik.items()}
        ref = pointwise_log_likelihood(Ah, yh, out["draws"][f], **like)["lppd"]
        got = out["elpd_cv_i"][held]
        worst_e = max(worst_e, float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()))
        mref = Ah @ out["draws"][f].reshape(-1, A.shape[1] + 1)[:, :-1].mean(axis=0)
        worst_m = max(worst_m, float(np.abs(out["cv_mean_i"][held] - mref).max() / np.abs(mref).max()))
    return worst_e, worst_m


def check_summary(y, folds, F, out, n_draws):
    ref = cv.cv_summary(y, folds, F, out["elpd_cv_i"], out["cv_mean_i"], n_draws)
    for key in ("elpd_cv", "se", "cv_rmse"):
        assert out[key] == pytest.approx(ref[key], rel=1e-13)
    assert np.array_equal(out["n_fold"], ref["n_fold"]) and out["n_fold"].sum() == len(y)
    assert out["n_points"] == len(y) and out["n_folds"] == F and out["n_draws"] == n_draws


@pytest.mark.parametrize("name", list(CASES))
def test_scores_are_the_scoring_paths(name):
    A, y, prior, folds, F, C, nu, out = run(name)
    worst_e, worst_m = score_errors(A, y, folds, F, out, nu=nu)
    print(f"{name}: elpd_cv_i {worst_e:.3e} (bar {TOL_ELPD:.0e}), cv_mean_i {worst_m:.3e} (bar {TOL_MEAN:.0e})")
    assert worst_e <= TOL_ELPD and worst_m <= TOL_MEAN
    check_summary(y, folds, F, out, C * T)


def test_scores_with_a_nu_per_draw():
    A, y, prior, folds, F, C, out = run_estimate()
    worst_e, worst_m = score_errors(A, y, folds, F, out, nu_draws=out["nu_draws"])
    print(f"estimate: elpd_cv_i {worst_e:.3e} (bar {TOL_ELPD:.0e}), cv_mean_i {worst_m:.3e} (bar {TOL_MEAN:.0e})")
    assert worst_e <= TOL_ELPD and worst_m <= TOL_MEAN
    check_summary(y, folds, F, out, C * T)


def same(a, b):
    """The same keys and the same bits; NaN (the held-out rows of row_weights) equals NaN."""
    def eq(u, v):
        u, v = np.asarray(u), np.asarray(v)
        return np.array_equal(u, v, equal_nan=u.dtype.kind == "f")
    return set(a) == set(b) and all(eq(a[key], b[key]) for key in a)


def test_repeats_and_memory_orders_give_the_same_bits():
    A, y, prior, folds, F, C, nu, out = run("k3")
    kw = dict(n_chains=C, seed=5, nu=nu, return_draws=True, return_row_weights=True)
    assert same(out, cv.kfold_cv(A, y, prior, folds, T, **kw))
    assert same(out, cv.kfold_cv(np.asfortranarray(A), y, prior, folds, T, **kw))
    A, y, prior, folds, F, C, est = run_estimate()
    again = cv.kfold_cv(np.asfortranarray(A), y, prior, folds, T, n_chains=2, seed=6, nu="estimate",
                        nu_grid=GRID7, nu_prior=PRIOR7, nu_init=5.0, return_draws=True, return_row_weights=True)
    assert same(est, again)


def test_batches_of_folds_give_the_same_bits(monkeypatch):
    """A memory budget of the two largest folds: the four folds of k3 go in two batches, the three
    of the estimated case (unequal, largest first in bytes: fold 0) in two."""
    A, y, prior, folds, F, C, nu, out = run("k3")
    n, k = A.shape

    def fold_bytes(nt, k, C, grid):
        padded = -(-(-(-nt // 4)) // 4) * 16
        chain = (T * k + T + 3 * nt + 2 * T * (k + 1)) * 8 + (2 * T * 4 if grid else 0)
        return padded * 17 * 8 + C * chain + 4 * grid * 8

    monkeypatch.setenv("PYBMC_AMD_CV_MAX_BYTES", str(2 * fold_bytes(53, k, C, 0)))
    split = cv.kfold_cv(A, y, prior, folds, T, n_chains=C, seed=5, nu=nu, return_draws=True,
                        return_row_weights=True)
    assert same(out, split)
    A, y, prior, folds, F, C, est = run_estimate()
    monkeypatch.setenv("PYBMC_AMD_CV_MAX_BYTES", str(2 * fold_bytes(50, 3, 2, 7)))
    split = cv.kfold_cv(A, y, prior, folds, T, n_chains=2, seed=6, nu="estimate", nu_grid=GRID7,
                        nu_prior=PRIOR7, nu_init=5.0, return_draws=True, return_row_weights=True)
    assert same(est, split)
    # and a budget below one fold is refused, the context staying usable
    monkeypatch.setenv("PYBMC_AMD_CV_MAX_BYTES", "1000")
    with pytest.raises(MemoryError, match="bytes of device memory"):
        cv.kfold_cv(A, y, prior, folds, T, n_chains=2, seed=6, nu=4.0)
    monkeypatch.delenv("PYBMC_AMD_CV_MAX_BYTES")
    assert np.isfinite(cv.kfold_cv(A, y, prior, folds, T, n_chains=2, seed=6, nu=4.0)["elpd_cv"])


def test_burn_and_thin_select_the_kept_draws():
    A, y, prior, folds, F, C, nu, out = run("k3")
    thin = cv.kfold_cv(A, y, prior, folds, T, burn=7, thin=3, n_chains=C, seed=5, nu=nu, return_draws=True)
    assert np.array_equal(thin["draws"], out["draws"][:, :, 7::3])
    assert thin["n_draws"] == C * out["draws"][:, :, 7::3].shape[2]
    worst_e, worst_m = score_errors(A, y, folds, F, thin, nu=nu)
    assert worst_e <= TOL_ELPD and worst_m <= TOL_MEAN
    A, y, prior, folds, F, C, est = run_estimate()
    thin = cv.kfold_cv(A, y, prior, folds, T, burn=7, thin=3, n_chains=2, seed=6, nu="estimate", nu_grid=GRID7,
                       nu_prior=PRIOR7, nu_init=5.0, return_draws=True)
    assert np.array_equal(thin["draws"], est["draws"][:, :, 7::3])
    assert np.array_equal(thin["nu_draws"], est["nu_draws"][:, :, 7::3])
    worst_e, worst_m = score_errors(A, y, folds, F, thin, nu_draws=thin["nu_draws"])
    assert worst_e <= TOL_ELPD and worst_m <= TOL_MEAN


def test_launch_split():
    """30 folds x 35 chains = 1050 workgroups: launches of 1024 and 26.  The call repeats bit for
    bit, and the chains on both sides of the split are their subset's chains."""
    n, k, F, C, sweeps = 60, 2, 30, 35, 20
    A, y, prior = problem(n, k, 9)
    folds = cv.fold_labels(n, F, seed=1)
    a = cv.kfold_cv(A, y, prior, folds, sweeps, n_chains=C, seed=9, nu=4.0, return_draws=True)
    b = cv.kfold_cv(A, y, prior, folds, sweeps, n_chains=C, seed=9, nu=4.0, return_draws=True)
    assert same(a, b)
    assert np.isfinite(a["draws"]).all() and np.isfinite(a["elpd_cv_i"]).all()
    for chain in (0, 1023, 1024, 1049):
        f, c = divmod(chain, C)
        ref, _ = solo(A, y, prior, folds, f, a["seeds"][f, c], 4.0, iters=sweeps)
        assert np.array_equal(a["draws"][f, c], ref), chain


def test_a_singular_fold_is_named():
    rng = np.random.default_rng(4)
    n, k = 120, 3
    A = rng.standard_normal((n, k))
    folds = np.arange(n) % 4
    A[folds != 2, 1] = 0.0            # column 1 lives in fold 2 alone: without it X'X is singular
    y = rng.standard_normal(n)
    with pytest.raises(BmcError, match="fold 2") as e:
        cv.kfold_cv(A, y, [np.zeros(k), np.eye(k), 1.0, 0.02], folds, 50, nu=4.0)
    assert isinstance(e.value, np.linalg.LinAlgError)
    # the context is usable afterwards
    A[:, 1] = rng.standard_normal(n)
    out = cv.kfold_cv(A, y, [np.zeros(k), np.eye(k), 1.0, 0.02], folds, 50, nu=4.0)
    assert np.isfinite(out["elpd_cv"])


def test_the_t_fit_wins_on_planted_outliers():
    """The 200 x 3 planted problem: exact 10-fold cross-validation prefers the Student-t fit to the
    Gaussian one by more than two standard errors of the difference, and in every fold that trains
    on a planted row that row's weight stays below the median weight of the clean rows.
    Measured on the MI355X: see the README's cross-validation row."""
    y, X, prior, beta_true, idx = RC.planted("200x3")
    n, k = X.shape
    folds = cv.fold_labels(n, 10, seed=2)
    kw = dict(burn=RC.PLANTED_BURN, n_chains=4, seed=21)
    sweeps = RC.PLANTED_BURN + RC.PLANTED_KEEP
    gauss = cv.kfold_cv(X, y, prior, folds, sweeps, **kw)
    t = cv.kfold_cv(X, y, prior, folds, sweeps, nu=4.0, return_row_weights=True, **kw)
    cmp = compare_elpd({"gauss": gauss, "t": t})
    ratio = cmp["elpd_diff"][1] / cmp["se_diff"][1]
    print(f"planted 200 x 3: elpd_cv t {t['elpd_cv']:.2f}, gauss {gauss['elpd_cv']:.2f}, "
          f"elpd_diff / se_diff = {ratio:.2f}")
    assert cmp["names"] == ["t", "gauss"] and cmp["kind"] == "elpd_cv_i"
    assert cmp["elpd_diff"][1] > 2.0 * cmp["se_diff"][1]
    clean = np.setdiff1d(np.arange(n), idx)
    w = t["row_weights"].mean(axis=1)                       # (F, n): the chains' mean
    for f in range(10):
        trained = idx[folds[idx] != f]
        med = np.median(w[f][clean[folds[clean] != f]])
        assert trained.size and (w[f][trained] < med).all(), f


def _standin_bmc():
    from pybmc_amd import BayesianModelCombination, Dataset
    models = ["FRDM", "HFB24", "UNEDF1", "SKM"]
    ds = Dataset(os.path.join(GOLDEN, "dataset_standin.csv"))
    data = ds.load_data(models + ["truth"], keys=["BE"], domain_keys=["N", "Z"])
    train_df, _, _ = ds.split_data(data, "BE", splitting_algorithm="random", train_size=0.6,
                                   val_size=0.2, test_size=0.2)
    b = BayesianModelCombination(models, data, truth_column_name="truth")
    b.orthogonalize("BE", train_df, components_kept=3, method="svd")
    return b, train_df


def test_validate_on_the_standin_dataset():
    b, train_df = _standin_bmc()
    n = len(train_df)
    opts = {"iterations": 400, "burn": 100, "n_chains": 2}
    # Gaussian options: cross_validate()'s result
    assert same(b.validate(n_folds=5, training_options=opts, seed=3),
                b.cross_validate(n_folds=5, training_options=opts, seed=3))
    # the t options: kfold_cv(nu=...) on U_hat, bit for bit, with cross_validate()'s extras
    out = b.validate(n_folds=5, training_options=dict(opts, sampler="student_t", nu=3.0), seed=3)
    U = np.asarray(b.U_hat, dtype=np.float64)
    yc = np.asarray(b.centered_experiment_train, dtype=np.float64)
    prior = [np.zeros(3), np.diag(b.S_hat ** 2), 1.0, 0.02]
    ref = cv.kfold_cv(U, yc, prior, cv.fold_labels(n, 5, 3), 400, burn=100, n_chains=2, seed=3, nu=3.0)
    assert all(np.array_equal(np.asarray(out[key]), np.asarray(ref[key])) for key in ref)
    assert out["likelihood"] == "student_t" and out["nu"] == 3.0 and out["n_draws"] == 2 * 300
    assert np.array_equal(out["folds"], cv.fold_labels(n, 5, 3))
    np.testing.assert_allclose(out["residual"], out["truth"] - out["predicted"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(out["truth"], train_df["truth"].to_numpy(), rtol=0, atol=1e-12)
    # after a Student-t train() the plain call takes that fit's likelihood; cross_validate() refuses
    b.train({"sampler": "student_t", "nu": 3.0, "iterations": 200, "seeds": [7]})
    assert same(out, b.validate(n_folds=5, training_options=opts, seed=3))
    with pytest.raises(ValueError, match="supports the Gaussian Gibbs sampler only"):
        b.cross_validate(n_folds=5, training_options=opts, seed=3)
    groups = b.validate(groups="Z", training_options=opts, seed=3)
    zs = np.unique(train_df["Z"].to_numpy())
    assert groups["n_folds"] == len(zs) and np.array_equal(groups["groups"], zs) and groups["nu"] == 3.0
