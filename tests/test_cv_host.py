"""CPU checks of pybmc_amd.cv: the fold labels, every argument error before a device is touched, the
host summary, and the numpy reference's total-minus-own training statistics against the subset's
own (what the device path relies on)."""
import numpy as np
import pytest

import cv_reference as CV
import pybmc_amd
from pybmc_amd import _lib, cv


def test_exports():
    assert callable(pybmc_amd.kfold_cv) and "kfold_cv" in pybmc_amd.__all__
    assert callable(pybmc_amd.fold_labels) and "fold_labels" in pybmc_amd.__all__
    assert hasattr(pybmc_amd.BayesianModelCombination, "cross_validate")


@pytest.mark.parametrize("n,F", [(150, 5), (629, 10), (7, 7), (1001, 3)])
def test_fold_labels_are_balanced_and_reproducible(n, F):
    a = cv.fold_labels(n, F, seed=3)
    assert a.dtype == np.int64 and a.shape == (n,)
    count = np.bincount(a, minlength=F)
    assert count.sum() == n and count.max() - count.min() <= 1 and count.min() >= 1
    assert np.array_equal(a, cv.fold_labels(n, F, seed=3))
    if n > 2 * F:
        assert not np.array_equal(a, cv.fold_labels(n, F, seed=4))
        assert not np.array_equal(a, np.arange(n) % F)          # shuffled, not striped
    with pytest.raises(ValueError):
        cv.fold_labels(n, n + 1)
    with pytest.raises(ValueError):
        cv.fold_labels(n, 1)


def test_group_labels():
    lab, groups = cv.group_labels(["Sn", "Pb", "Sn", "Ca", "Pb"])
    assert list(groups) == ["Ca", "Pb", "Sn"] and list(lab) == [2, 1, 2, 0, 1] and lab.dtype == np.int64
    lab, groups = cv.group_labels(np.array([50, 82, 50, 20]))
    assert list(groups[lab]) == [50, 82, 50, 20]


@pytest.mark.parametrize("name,F", [("unequal", 5), ("tight", 3)])
def test_total_minus_own_is_the_subset_statistic(name, F):
    """150 x 3 / F = 5 and 90 x 17 / F = 3: the training X'X and X'y of every fold from one Gram per
    fold equal those computed on the subset itself to 1e-13 relative."""
    A, y, prior, folds, F_, C = CV.case(name)
    assert F_ == F and A.shape == CV.CASES[name][:2]
    if name == "unequal":
        assert np.bincount(folds).min() == 1
    XtX, Xty = CV.fold_statistics(A, y, folds, F)
    for f in range(F):
        st = CV.subset_setup(A, y, prior, folds, f)
        tr = folds != f
        assert st["n"] == int(tr.sum())
        assert np.abs(XtX[f] - st["XtX"]).max() <= 1e-13 * np.abs(st["XtX"]).max()
        direct = A[tr].T @ y[tr]
        assert np.abs(Xty[f] - direct).max() <= 1e-13 * np.abs(direct).max()


def test_reference_scores_only_the_held_out_rows_of_a_fold():
    A, y, prior, folds, F, C = CV.case("unequal")
    rng = np.random.default_rng(0)
    k = A.shape[1]
    draws = np.concatenate([rng.standard_normal((F, C, 40, k)), 0.5 + rng.random((F, C, 40, 1))], axis=-1)
    elpd, mean = CV.cv_reference(A, y, folds, F, draws)
    other = draws.copy()
    other[2] += 1.0                                      # another posterior for fold 2 alone
    elpd2, mean2 = CV.cv_reference(A, y, folds, F, other)
    moved = folds == 2
    assert np.array_equal(elpd[~moved], elpd2[~moved]) and np.array_equal(mean[~moved], mean2[~moved])
    assert (elpd[moved] != elpd2[moved]).all()
    got = cv.cv_summary(y, folds, F, elpd, mean, C * 40)
    ref = CV.summary(y, folds, F, elpd, mean)
    for key in ("elpd_cv", "se", "cv_rmse"):
        assert got[key] == pytest.approx(ref[key], rel=1e-13)
    assert np.allclose(got["elpd_fold"], ref["elpd_fold"], rtol=1e-13, atol=0)
    assert np.array_equal(got["n_fold"], ref["n_fold"]) and got["n_fold"].sum() == len(y)
    assert got["n_points"] == len(y) and got["n_folds"] == F and got["n_draws"] == C * 40


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a context was asked for before the arguments were checked")
    monkeypatch.setattr(_lib, "default_context", refuse)


def test_argument_errors_need_no_gpu(no_device):
    rng = np.random.default_rng(1)
    n, k = 40, 3
    A = rng.standard_normal((n, k))
    y = rng.standard_normal(n)
    prior = [np.zeros(k), np.eye(k), 1.0, 0.02]
    folds = np.arange(n) % 4

    def call(A=A, y=y, prior=prior, folds=folds, iterations=50, **kw):
        return cv.kfold_cv(A, y, prior, folds, iterations, **kw)

    with pytest.raises(ValueError, match="integer"):
        call(folds=folds.astype(float))
    with pytest.raises(ValueError, match="integer"):
        call(folds=folds % 2 == 0)
    with pytest.raises(ValueError, match="negative"):
        call(folds=folds - 1)
    with pytest.raises(ValueError, match="folds must be"):
        call(folds=folds[:-1])
    with pytest.raises(ValueError, match="fold 2 is empty"):
        call(folds=np.where(folds == 2, 0, folds))
    with pytest.raises(ValueError, match="between 2 and 1024 folds"):
        call(folds=np.zeros(n, dtype=int))
    big = rng.standard_normal((1100, 1))
    with pytest.raises(ValueError, match="between 2 and 1024 folds"):
        call(A=big, y=big[:, 0].copy(), prior=[np.zeros(1), np.eye(1), 1.0, 0.02], folds=np.arange(1100) % 1025)
    # a fold whose training set has fewer than k rows
    with pytest.raises(ValueError, match="fold 0: its training set has 2 rows"):
        call(folds=np.array([0] * (n - 2) + [1, 1]))
    wide = rng.standard_normal((200, 65))
    with pytest.raises(ValueError, match="at most 64"):
        call(A=wide, y=rng.standard_normal(200), prior=[np.zeros(65), np.eye(65), 1.0, 0.02],
             folds=np.arange(200) % 2)
    # the shape checks of scoring._check_shapes
    with pytest.raises(ValueError, match="A must be"):
        call(A=A[:, 0])
    with pytest.raises(ValueError, match="y must be"):
        call(y=y[:-1])
    with pytest.raises(ValueError, match="burn"):
        call(burn=-1)
    with pytest.raises(ValueError, match="thin"):
        call(thin=0)
    with pytest.raises(ValueError, match="at least 2 draws"):
        call(iterations=10, burn=9)
    with pytest.raises(ValueError, match="float64"):
        call(A=A.astype(np.float32))
    with pytest.raises(ValueError, match="iterations"):
        call(iterations=0)
    with pytest.raises(ValueError, match="n_chains"):
        call(n_chains=0)
    with pytest.raises(ValueError, match="prior_info"):
        call(prior=[np.zeros(k + 1), np.eye(k), 1.0, 0.02])
    with pytest.raises(ValueError, match="not both"):
        call(seed=1, seeds=np.ones((4, 1), dtype=np.uint64))
    with pytest.raises(ValueError, match="seeds must be"):
        call(seeds=np.ones(4, dtype=np.uint64), n_chains=2)


def test_seeds_follow_the_chain_rule():
    from pybmc_amd.chains import chain_seeds
    s = cv._check_seeds(11, None, 5, 3)
    assert s.shape == (5, 3) and s.dtype == np.uint64
    assert s[2, 1] == chain_seeds(11, [2 * 3 + 1])[0]
    given = np.arange(15, dtype=np.uint64).reshape(5, 3)
    assert np.array_equal(cv._check_seeds(None, given, 5, 3), given)


def test_cross_validate_refuses_the_simplex_sampler_and_bad_groups(no_device):
    import pandas as pd
    rng = np.random.default_rng(2)
    df = pd.DataFrame(rng.standard_normal((30, 3)), columns=["m0", "m1", "m2"])
    df["truth"] = rng.standard_normal(30)
    df["Z"] = np.arange(30) % 5
    bmc = pybmc_amd.BayesianModelCombination(["m0", "m1", "m2"], {"p": df}, "truth")
    with pytest.raises(ValueError, match="orthogonalize"):
        bmc.cross_validate()
    bmc.orthogonalize("p", df, 2, method="svd")
    with pytest.raises(ValueError, match="simplex"):
        bmc.cross_validate(training_options={"sampler": "simplex"})
    with pytest.raises(ValueError, match="no column"):
        bmc.cross_validate(groups="N")
    with pytest.raises(ValueError, match="one entry per training row"):
        bmc.cross_validate(groups=np.arange(29))
