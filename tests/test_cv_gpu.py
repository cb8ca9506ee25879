"""Exact K-fold / leave-group-out cross-validation on the device (-m gpu): pybmc_amd.cv.kfold_cv and
BayesianModelCombination.cross_validate.

Bars (none taken from the code under test):
  chains   every CV chain against gibbs_sampler on the training subset under the same seed, the
           data-pass loop: 1e-8 x the column's scale, the bar test_gram_mode_gpu.py holds between the
           two rss modes (a CV chain differs from it through the rounding of rss and of the
           total-minus-own Gram only);
  scores   elpd_cv_i against pointwise_log_likelihood on the held-out rows and the fold's draws:
           1e-11 max(1, |ref|), the bar of test_scoring_gpu.py; cv_mean_i against A @ mean(draws):
           1e-12 relative to the largest |mean| (two float64 summation orders of <= 600 draws);
  repeats  bit for bit.
Measured on the MI355X: chains 5.8e-15 / 9.7e-16 / 3.1e-14 / 2.1e-13 / 4.2e-11 (unequal, one_col, tight,
wide, tight_scaled), launch split 8.5e-16; elpd_cv_i 0 everywhere; cv_mean_i at most 9.5e-16."""
import os

import numpy as np
import pytest

import cv_reference as CV
from pybmc_amd import cv, gibbs_sampler, pointwise_log_likelihood
from pybmc_amd._lib import BmcError

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL_CHAIN, TOL_ELPD, TOL_MEAN = 1e-8, 1e-11, 1e-12
_runs = {}


def run(name):
    """One kfold_cv call per case, shared by the tests and left unchanged."""
    if name not in _runs:
        A, y, prior, folds, F, C = CV.case(name)
        out = cv.kfold_cv(A, y, prior, folds, CV.T, n_chains=C, seed=5, return_draws=True)
        _runs[name] = (A, y, prior, folds, F, C, out)
    return _runs[name]


def chain_error(draws, A, y, prior, folds, f, seed, T):
    """max over the columns of |CV chain - subset chain| / column scale"""
    tr = folds != f
    ref = gibbs_sampler(y[tr], np.ascontiguousarray(A[tr]), T, prior, seeds=[seed])
    scale = np.abs(ref).max(axis=0)
    return float((np.abs(draws - ref).max(axis=0) / scale).max())


@pytest.mark.parametrize("name", list(CV.CASES))
def test_chains_are_the_subsets_chains(name):
    A, y, prior, folds, F, C, out = run(name)
    n, k = A.shape
    assert out["draws"].shape == (F, C, CV.T, k + 1) and out["seeds"].shape == (F, C)
    assert np.isfinite(out["draws"]).all()
    worst = 0.0
    for f in range(F):
        for c in range(C):
            worst = max(worst, chain_error(out["draws"][f, c], A, y, prior, folds, f, out["seeds"][f, c], CV.T))
    print(f"{name}: worst chain difference / column scale = {worst:.3e} (bar {TOL_CHAIN:.0e})")
    assert worst < TOL_CHAIN
    if name == "tight_scaled":
        # no floor binds here, so sigma is the data's: n_train = 60 rows, 17 coefficients and the
        # gamma shape (nu0 + n_train) / 2 put E sigma^2 near 43/59 of the true one (sigma x 0.85); a
        # cancelled rss0 would be off by orders of magnitude
        n, k, _, _, snr = CV.CASES[name]
        sig = CV.problem(n, k, snr, CV.SCALE[name])[3]
        assert sig ** 2 > 1e-5 and 0.5 < out["draws"][..., -1].mean() / sig < 1.5


@pytest.mark.parametrize("name", list(CV.CASES))
def test_scores_are_the_scoring_paths(name):
    A, y, prior, folds, F, C, out = run(name)
    worst_e = worst_m = 0.0
    for f in range(F):
        held = folds == f
        Ah, yh = np.ascontiguousarray(A[held]), y[held]
        ref = pointwise_log_likelihood(Ah, yh, out["draws"][f])["lppd"]
        got = out["elpd_cv_i"][held]
        worst_e = max(worst_e, float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()))
        mref = Ah @ out["draws"][f].reshape(-1, A.shape[1] + 1)[:, :-1].mean(axis=0)
        worst_m = max(worst_m, float(np.abs(out["cv_mean_i"][held] - mref).max() / np.abs(mref).max()))
    print(f"{name}: elpd_cv_i {worst_e:.3e} (bar {TOL_ELPD:.0e}), cv_mean_i {worst_m:.3e} (bar {TOL_MEAN:.0e})")
    assert worst_e <= TOL_ELPD and worst_m <= TOL_MEAN
    # and the dense numpy reference, with the summary
    elpd, mean = CV.cv_reference(A, y, folds, F, out["draws"])
    assert (np.abs(out["elpd_cv_i"] - elpd) <= TOL_ELPD * np.maximum(1.0, np.abs(elpd))).all()
    ref = CV.summary(y, folds, F, out["elpd_cv_i"], out["cv_mean_i"])
    for key in ("elpd_cv", "se", "cv_rmse"):
        assert out[key] == pytest.approx(ref[key], rel=1e-13)
    assert np.array_equal(out["n_fold"], ref["n_fold"]) and out["n_fold"].sum() == len(y)
    assert out["n_points"] == len(y) and out["n_folds"] == F and out["n_draws"] == C * CV.T


def same(a, b):
    return all(np.array_equal(np.asarray(a[key]), np.asarray(b[key])) for key in a)


def test_repeatable_bit_for_bit():
    A, y, prior, folds, F, C, out = run("unequal")
    again = cv.kfold_cv(A, y, prior, folds, CV.T, n_chains=C, seed=5, return_draws=True)
    assert set(again) == set(out) and same(out, again)
    # a Fortran-ordered A (U_hat's layout) is the same problem
    fort = cv.kfold_cv(np.asfortranarray(A), y, prior, folds, CV.T, n_chains=C, seed=5, return_draws=True)
    assert same(out, fort)


def test_burn_and_thin_select_the_kept_draws():
    A, y, prior, folds, F, C, out = run("unequal")
    thin = cv.kfold_cv(A, y, prior, folds, CV.T, burn=37, thin=4, n_chains=C, seed=5, return_draws=True)
    assert np.array_equal(thin["draws"], out["draws"][:, :, 37::4])
    assert thin["n_draws"] == C * out["draws"][:, :, 37::4].shape[2]
    held = folds == 3
    ref = pointwise_log_likelihood(np.ascontiguousarray(A[held]), y[held], thin["draws"][3])["lppd"]
    assert (np.abs(thin["elpd_cv_i"][held] - ref) <= TOL_ELPD * np.maximum(1.0, np.abs(ref))).all()


def test_batches_of_folds_give_the_same_bits(monkeypatch):
    """A memory budget of two folds' chains at a time: four batches instead of one."""
    A, y, prior, folds, F, C, out = run("one_col")
    k = A.shape[1]
    per_fold = C * (CV.T * k + CV.T + 2 * CV.T * (k + 1)) * 8
    monkeypatch.setenv("PYBMC_AMD_CV_MAX_BYTES", str(2 * per_fold + 100))
    split = cv.kfold_cv(A, y, prior, folds, CV.T, n_chains=C, seed=5, return_draws=True)
    assert same(out, split)


def test_launch_split():
    """30 folds x 70 chains = 2100 one-wave chains: launches of 2048 and 52.  The call repeats bit
    for bit, and the chains on both sides of the split are their subset's chains."""
    n, k, F, C, T = 200, 2, 30, 70, 20
    A, y, prior, _ = CV.problem(n, k, 10.0)
    folds = cv.fold_labels(n, F, seed=1)
    a = cv.kfold_cv(A, y, prior, folds, T, n_chains=C, seed=9, return_draws=True)
    b = cv.kfold_cv(A, y, prior, folds, T, n_chains=C, seed=9, return_draws=True)
    assert same(a, b)
    assert np.isfinite(a["draws"]).all() and np.isfinite(a["elpd_cv_i"]).all()
    worst = 0.0
    for chain in (0, 2047, 2048, 2099):
        f, c = divmod(chain, C)
        worst = max(worst, chain_error(a["draws"][f, c], A, y, prior, folds, f, a["seeds"][f, c], T))
    print(f"launch split: worst chain difference / column scale = {worst:.3e} (bar {TOL_CHAIN:.0e})")
    assert worst < TOL_CHAIN


def test_a_singular_fold_is_named():
    rng = np.random.default_rng(4)
    n, k = 120, 3
    A = rng.standard_normal((n, k))
    folds = np.arange(n) % 4
    A[folds != 2, 1] = 0.0            # column 1 lives in fold 2 alone: without it X'X is singular
    y = rng.standard_normal(n)
    with pytest.raises(BmcError, match="fold 2") as e:
        cv.kfold_cv(A, y, [np.zeros(k), np.eye(k), 1.0, 0.02], folds, 50)
    assert isinstance(e.value, np.linalg.LinAlgError)
    # the context is usable afterwards
    A[:, 1] = rng.standard_normal(n)
    out = cv.kfold_cv(A, y, [np.zeros(k), np.eye(k), 1.0, 0.02], folds, 50)
    assert np.isfinite(out["elpd_cv"])


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


def test_cross_validate_on_the_standin_dataset():
    b, train_df = _standin_bmc()
    n = len(train_df)
    opts = {"iterations": 400, "burn": 100, "n_chains": 2}
    out = b.cross_validate(n_folds=5, training_options=opts, seed=3)
    assert out["n_folds"] == 5 and out["n_points"] == n and out["n_draws"] == 2 * 300
    assert out["n_fold"].sum() == n and out["n_fold"].max() - out["n_fold"].min() <= 1
    for key in ("elpd_cv_i", "cv_mean_i", "predicted", "truth", "residual", "folds"):
        assert out[key].shape == (n,)
    assert np.isfinite(out["elpd_cv"]) and np.isfinite(out["se"]) and out["cv_rmse"] > 0
    np.testing.assert_allclose(out["residual"], out["truth"] - out["predicted"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(out["truth"], train_df["truth"].to_numpy(), rtol=0, atol=1e-12)
    assert out["elpd_fold"].sum() == pytest.approx(out["elpd_cv"], rel=1e-12)
    assert same(out, b.cross_validate(n_folds=5, training_options=opts, seed=3))
    # leave-group-out: one fold per isotopic chain, by column name and by array
    by_name = b.cross_validate(groups="Z", training_options=opts, seed=3)
    zs = np.unique(train_df["Z"].to_numpy())
    assert by_name["n_folds"] == len(zs) and np.array_equal(by_name["groups"], zs)
    assert np.array_equal(by_name["groups"][by_name["folds"]], train_df["Z"].to_numpy())
    assert np.array_equal(by_name["n_fold"], np.bincount(by_name["folds"])) and by_name["n_fold"].sum() == n
    by_array = b.cross_validate(groups=train_df["Z"].to_numpy(), training_options=opts, seed=3)
    assert same(by_name, by_array)
    with pytest.raises(ValueError, match="simplex"):
        b.cross_validate(training_options={"sampler": "simplex"})
