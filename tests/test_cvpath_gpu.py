"""The component path on the device (-m gpu): pybmc_amd.cv.cv_component_path and
BayesianModelCombination.component_path.

Bars (none taken from the code under test):
  path     every candidate k against kfold_cv on A[:, :k] under the same seeds: np.array_equal.  Every
           stage is the same computation: a Gram entry is a dot product over the rows in fixed chunk
           order whatever tile its columns fall in, total - own and the k x k algebra see the same
           numbers, a zero-padded rss term leaves the accumulator alone, the variates come from the
           same launch_rng_fill call and the chain body is the same instantiation;
  chains   every chain against gibbs_sampler on the training rows and leading k columns under the
           same seed: 1e-8 x the column's scale (the bar of test_cv_gpu.py);
  scores   elpd_cv_i against pointwise_log_likelihood on the held-out rows and the fold's draws:
           1e-11 max(1, |ref|); cv_mean_i against A[held, :k] @ mean(draws): 1e-12 relative to the
           largest |mean|;
  summary  against cv_reference.summary, rel 1e-13, and path_summary recomputed;
  repeats  bit for bit.
Measured on the MI355X: no element of any candidate's draws, elpd_cv_i or cv_mean_i differs from
kfold_cv's in any case; chains 5.8e-15 / 2.1e-13 / 4.2e-11 / 4.1e-16 (small, edges, tight, split);
elpd_cv_i 0 everywhere; cv_mean_i at most 1.8e-15; the selection test gives elpd_cv 8.28, 69.63,
110.94, 109.08, 108.69, 108.31 and se_diff 8.36, 6.95, 0, 0.70, 0.67, 0.90 (k_best 3, k_1se 3).
"""
import os

import numpy as np
import pytest

import cv_reference as CV
from pybmc_amd import cv, gibbs_sampler, pointwise_log_likelihood
from pybmc_amd._lib import BmcError, SingularFoldError

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL_CHAIN, TOL_ELPD, TOL_MEAN = 1e-8, 1e-11, 1e-12


def balanced(n, F):
    return np.random.default_rng(n).permutation(np.arange(n) % F).astype(np.int64)


def make_case(name):
    """(A, y, prior, folds, C, T, components or None, chains to hold against gibbs_sampler or None)"""
    if name == "small":
        A, y, prior, _ = CV.problem(150, 3, 10.0)
        return A, y, prior, CV.unequal_folds(150, 5, 7), 2, CV.T, None, None
    if name == "edges":
        A, y, prior, _ = CV.problem(1300, 64, 10.0)
        return A, y, prior, balanced(1300, 2), 1, CV.T, (1, 8, 9, 16, 17, 32, 33, 64), None
    if name == "tight":
        A, y, prior, _ = CV.problem(90, 17, 1e5, scale=1e3)
        return A, y, prior, balanced(90, 3), 1, CV.T, (5, 17), None
    if name == "split":
        A, y, prior, _ = CV.problem(200, 2, 10.0)
        return A, y, prior, cv.fold_labels(200, 30, 1), 40, 20, (1, 2), (0, 2047, 2048, 2399)
    raise KeyError(name)


CASES = ("small", "edges", "tight", "split")
_runs = {}


def sub_prior(prior, k):
    b0, C0, nu0, s20 = prior
    return [b0[:k], C0[:k, :k], nu0, s20]


def run(name):
    """One cv_component_path call per case and the kfold_cv call of every candidate, shared by the
    tests and left unchanged."""
    if name not in _runs:
        A, y, prior, folds, C, T, comps, picks = make_case(name)
        out = cv.cv_component_path(A, y, prior, folds, T, components=comps, n_chains=C, seed=5,
                                   return_draws=True)
        singles = [cv.kfold_cv(np.ascontiguousarray(A[:, :k]), y, sub_prior(prior, k), folds, T, n_chains=C,
                               seeds=out["seeds"], return_draws=True) for k in out["components"]]
        _runs[name] = (A, y, prior, folds, C, T, comps, picks, out, singles)
    return _runs[name]


@pytest.mark.parametrize("name", CASES)
def test_every_candidate_is_the_existing_paths_result(name):
    A, y, prior, folds, C, T, comps, picks, out, singles = run(name)
    want = np.arange(1, A.shape[1] + 1) if comps is None else np.asarray(comps)
    assert np.array_equal(out["components"], want)
    F = int(folds.max()) + 1
    m, n = len(want), len(y)
    assert out["elpd_cv_i"].shape == (m, n) and out["cv_mean_i"].shape == (m, n)
    assert out["elpd_fold"].shape == (m, F) and out["seeds"].shape == (F, C)
    for j, k in enumerate(out["components"]):
        one = singles[j]
        assert out["draws"][j].shape == (F, C, T, k + 1)
        for key, got in (("draws", out["draws"][j]), ("elpd_cv_i", out["elpd_cv_i"][j]),
                         ("cv_mean_i", out["cv_mean_i"][j])):
            differ = int((np.asarray(got) != one[key]).sum())
            print(f"{name} k={k} {key}: {differ} of {one[key].size} elements differ from kfold_cv")
        assert np.array_equal(out["draws"][j], one["draws"])
        assert np.array_equal(out["elpd_cv_i"][j], one["elpd_cv_i"])
        assert np.array_equal(out["cv_mean_i"][j], one["cv_mean_i"])


def chain_error(draws, A, y, prior, folds, f, seed, T):
    tr = folds != f
    ref = gibbs_sampler(y[tr], np.ascontiguousarray(A[tr]), T, prior, seeds=[seed])
    scale = np.abs(ref).max(axis=0)
    return float((np.abs(draws - ref).max(axis=0) / scale).max())


@pytest.mark.parametrize("name", CASES)
def test_chains_are_the_subsets_chains(name):
    A, y, prior, folds, C, T, comps, picks, out, singles = run(name)
    F = int(folds.max()) + 1
    worst = 0.0
    for j, k in enumerate(out["components"]):
        assert np.isfinite(out["draws"][j]).all()
        Ak, pk = np.ascontiguousarray(A[:, :k]), sub_prior(prior, k)
        chains = [divmod(g, C) for g in range(F * C)] if picks is None else \
            [divmod(g - j * F * C, C) for g in picks if j * F * C <= g < (j + 1) * F * C]
        for f, c in chains:
            worst = max(worst, chain_error(out["draws"][j][f, c], Ak, y, pk, folds, f, out["seeds"][f, c], T))
    print(f"{name}: worst chain difference / column scale = {worst:.3e} (bar {TOL_CHAIN:.0e})")
    assert worst < TOL_CHAIN


@pytest.mark.parametrize("name", CASES)
def test_scores_and_summaries(name):
    A, y, prior, folds, C, T, comps, picks, out, singles = run(name)
    F = int(folds.max()) + 1
    worst_e = worst_m = 0.0
    for j, k in enumerate(out["components"]):
        for f in range(F):
            held = folds == f
            Ah, yh = np.ascontiguousarray(A[held, :k]), y[held]
            ref = pointwise_log_likelihood(Ah, yh, out["draws"][j][f])["lppd"]
            got = out["elpd_cv_i"][j][held]
            worst_e = max(worst_e, float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()))
            mref = Ah @ out["draws"][j][f].reshape(-1, k + 1)[:, :-1].mean(axis=0)
            worst_m = max(worst_m, float(np.abs(out["cv_mean_i"][j][held] - mref).max() / np.abs(mref).max()))
        ref = CV.summary(y, folds, F, out["elpd_cv_i"][j], out["cv_mean_i"][j])
        for key in ("elpd_cv", "se", "cv_rmse"):
            assert out[key][j] == pytest.approx(ref[key], rel=1e-13)
        assert out["elpd_fold"][j] == pytest.approx(ref["elpd_fold"], rel=1e-13)
    print(f"{name}: elpd_cv_i {worst_e:.3e} (bar {TOL_ELPD:.0e}), cv_mean_i {worst_m:.3e} (bar {TOL_MEAN:.0e})")
    assert worst_e <= TOL_ELPD and worst_m <= TOL_MEAN
    assert np.array_equal(out["n_fold"], np.bincount(folds)) and out["n_points"] == len(y)
    assert out["n_folds"] == F and out["n_draws"] == C * T
    sel = cv.path_summary(out["components"], out["elpd_cv_i"])
    assert out["k_best"] == sel["k_best"] and out["k_1se"] == sel["k_1se"]
    assert np.array_equal(out["elpd_diff"], sel["elpd_diff"]) and np.array_equal(out["se_diff"], sel["se_diff"])


def same(a, b):
    def eq(x, y):
        if isinstance(x, list):
            return len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y))
        return np.array_equal(np.asarray(x), np.asarray(y))
    return set(a) == set(b) and all(eq(a[key], b[key]) for key in a)


def test_repeatable_bit_for_bit():
    A, y, prior, folds, C, T, comps, picks, out, _ = run("small")
    again = cv.cv_component_path(A, y, prior, folds, T, n_chains=C, seed=5, return_draws=True)
    assert same(out, again)
    fort = cv.cv_component_path(np.asfortranarray(A), y, prior, folds, T, n_chains=C, seed=5, return_draws=True)
    assert same(out, fort)


def test_batches_of_problems_give_the_same_bits(monkeypatch):
    """A memory budget of just over two of the largest problems: several batches instead of one."""
    A, y, prior, folds, C, T, comps, picks, out, _ = run("small")
    k = A.shape[1]
    per_problem = C * (T * k + T + 2 * T * (k + 1)) * 8
    monkeypatch.setenv("PYBMC_AMD_CV_MAX_BYTES", str(2 * per_problem + 100))
    split = cv.cv_component_path(A, y, prior, folds, T, n_chains=C, seed=5, return_draws=True)
    assert same(out, split)


def test_burn_and_thin_select_the_kept_draws():
    A, y, prior, folds, C, T, comps, picks, out, _ = run("small")
    thin = cv.cv_component_path(A, y, prior, folds, T, burn=37, thin=4, n_chains=C, seed=5, return_draws=True)
    for j in range(len(out["components"])):
        assert np.array_equal(thin["draws"][j], out["draws"][j][:, :, 37::4])
    assert thin["n_draws"] == C * out["draws"][0][:, :, 37::4].shape[2]


def test_a_singular_candidate_is_named():
    rng = np.random.default_rng(4)
    n, k = 120, 3
    A = rng.standard_normal((n, k))
    folds = np.arange(n) % 4
    A[folds != 2, 1] = 0.0            # column 1 lives in fold 2 alone: candidates k >= 2 are singular there
    y = rng.standard_normal(n)
    prior = [np.zeros(k), np.eye(k), 1.0, 0.02]
    with pytest.raises(SingularFoldError, match=r"fold 2, 2 components") as e:
        cv.cv_component_path(A, y, prior, folds, 50)
    assert isinstance(e.value, BmcError) and isinstance(e.value, np.linalg.LinAlgError)
    with pytest.raises(SingularFoldError, match=r"fold 2, 3 components"):
        cv.cv_component_path(A, y, prior, folds, 50, components=(1, 3))
    out = cv.cv_component_path(A, y, prior, folds, 50, components=(1,))
    assert np.isfinite(out["elpd_cv"]).all() and out["k_best"] == 1


def test_selection_finds_the_true_size():
    """Three true components among six orthonormal columns.  The numpy oracle of this repository
    (gibbs_replay per training subset, score_reference.pointwise on the held-out rows) gives
    elpd_cv = 8.2, 69.6, 110.7, 109.1, 108.7, 108.0 for k = 1 .. 6 and se_diff = 8.4, 7.0, 0, 0.62,
    0.69, 0.96: the step from 2 to 3 is 41 against 7, the differences beyond 3 about one se_diff."""
    rng = np.random.default_rng(0)
    Q = np.linalg.qr(rng.standard_normal((120, 6)))[0]
    S = np.sort(rng.uniform(1.0, 3.0, 6))[::-1]
    beta = np.zeros(6)
    beta[:3] = S[:3] * np.array([1.0, -0.8, 0.6])
    sig = np.linalg.norm(Q @ beta) / np.sqrt(120) / 3.0
    y = Q @ beta + sig * rng.standard_normal(120)
    folds = np.random.default_rng(1).permutation(np.arange(120) % 5)
    prior = [np.zeros(6), np.diag(S ** 2), 1.0, 0.02]
    out = cv.cv_component_path(Q, y, prior, folds, 300, burn=50, n_chains=2, seed=0)
    print("elpd_cv", np.round(out["elpd_cv"], 2), "se_diff", np.round(out["se_diff"], 2),
          "k_best", out["k_best"], "k_1se", out["k_1se"])
    assert out["k_1se"] == 3
    assert out["elpd_cv"][2] - out["elpd_cv"][1] > 3 * out["se_diff"][1]


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


def test_component_path_on_the_standin_dataset():
    b, train_df = _standin_bmc()
    opts = {"iterations": 300, "burn": 50}
    out = b.component_path(n_folds=5, seed=11, training_options=opts)
    one = b.cross_validate(n_folds=5, seed=11, training_options=opts)
    table = out["table"]
    assert list(table.index) == [1, 2, 3]
    assert list(table.columns) == ["elpd_cv", "se", "elpd_diff", "se_diff", "cv_rmse"]
    assert np.array_equal(out["folds"], one["folds"])
    assert np.array_equal(out["elpd_cv_i"][2], one["elpd_cv_i"])
    assert np.array_equal(out["cv_mean_i"][2], one["cv_mean_i"])
    for key in ("elpd_cv", "se", "cv_rmse"):
        assert table.loc[3, key] == one[key]
    assert out["k_best"] in (1, 2, 3) and out["k_1se"] <= out["k_best"]
    by_name = b.component_path(groups="Z", components=(1, 3), seed=11, training_options=opts)
    ref = b.cross_validate(groups="Z", seed=11, training_options=opts)
    assert np.array_equal(by_name["folds"], ref["folds"]) and np.array_equal(by_name["groups"], ref["groups"])
    assert list(by_name["table"].index) == [1, 3]
    assert np.array_equal(by_name["elpd_cv_i"][1], ref["elpd_cv_i"])
