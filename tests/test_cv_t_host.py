"""Student-t cross-validation without a GPU: the argument checks of ``cv.kfold_cv(nu=...)`` (all
before any device work), which entry point the arguments select, and the dispatch of
``BayesianModelCombination.validate`` -- while ``cross_validate()`` and ``component_path()`` keep
refusing a Student-t fit."""
import threading

import numpy as np
import pytest

from pybmc_amd import _lib, cv
from pybmc_amd.inference_utils import robust_nu_prior


def problem(n=40, k=3, seed=0):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, k))
    y = A @ rng.standard_normal(k) + 0.1 * rng.standard_normal(n)
    return A, y, [np.zeros(k), np.eye(k), 1.0, 0.02], np.arange(n) % 4


def test_arguments_are_checked_before_any_device_work(monkeypatch):
    def no_device(*a, **kw):
        raise AssertionError("argument errors must be raised before any device work")

    monkeypatch.setattr(_lib, "default_context", no_device)
    A, y, prior, folds = problem()
    rng = np.random.default_rng(1)
    wide = rng.standard_normal((80, 33))
    with pytest.raises(ValueError, match="at most 32 columns; got 33"):
        cv.kfold_cv(wide, rng.standard_normal(80), [np.zeros(33), np.eye(33), 1.0, 0.02], np.arange(80) % 2, 10,
                    nu=4.0)
    for nu in (0, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="nu must be positive and finite"):
            cv.kfold_cv(A, y, prior, folds, 10, nu=nu)
    with pytest.raises(ValueError, match='a positive number or "estimate"'):
        cv.kfold_cv(A, y, prior, folds, 10, nu="free")
    for grid_arg in ({"nu_grid": [1.0, 2.0]}, {"nu_prior": [1.0]}, {"nu_init": 2.0}):
        with pytest.raises(ValueError, match='need nu="estimate"'):
            cv.kfold_cv(A, y, prior, folds, 10, nu=4.0, **grid_arg)
        with pytest.raises(ValueError, match="need nu"):
            cv.kfold_cv(A, y, prior, folds, 10, **grid_arg)
    with pytest.raises(ValueError, match="need nu"):
        cv.kfold_cv(A, y, prior, folds, 10, return_row_weights=True)
    with pytest.raises(ValueError, match="strictly increasing"):
        cv.kfold_cv(A, y, prior, folds, 10, nu="estimate", nu_grid=[2.0, 1.0])
    with pytest.raises(ValueError, match="nu_init must be a value of nu_grid"):
        cv.kfold_cv(A, y, prior, folds, 10, nu="estimate", nu_grid=[1.0, 2.0], nu_init=3.0)
    for nu in (4.0, "estimate"):
        with pytest.raises(ValueError, match="burn"):
            cv.kfold_cv(A, y, prior, folds, 10, burn=10, nu=nu)
        with pytest.raises(ValueError, match="burn = 12"):
            cv.kfold_cv(A, y, prior, folds, 10, burn=12, n_chains=4, nu=nu)
        with pytest.raises(ValueError, match="fold 1 is empty"):
            cv.kfold_cv(A, y, prior, np.where(folds == 1, 0, folds), 10, nu=nu)
        with pytest.raises(ValueError, match="float64"):
            cv.kfold_cv(A.astype(np.float32), y, prior, folds, 10, nu=nu)


class Ctx:
    """Records the call the arguments select and answers with arrays of the right shapes."""
    lock = threading.RLock()

    def __init__(self):
        self.calls = []

    def kfold_cv(self, A, n, k, lda, layout, y, fold, F, b0, C0, nu0, s20, C, T, burn, thin, seeds,
                 return_draws=False):
        self.calls.append(("gauss", {}))
        kept = -(-(T - burn) // thin)
        return np.zeros(n), np.zeros(n), np.zeros((F, C, kept, k + 1)) if return_draws else None

    def kfold_cv_t(self, A, n, k, lda, layout, y, fold, F, b0, C0, nu0, s20, C, T, burn, thin, seeds, **kw):
        self.calls.append(("t", kw))
        kept = -(-(T - burn) // thin)
        draws = np.zeros((F, C, kept, k + 1)) if kw["return_draws"] else None
        w = np.ones((F, C, n)) if kw["return_row_weights"] else None
        idx = np.full((F, C, kept), 2, dtype=np.int32) if kw["nu_grid"] is not None else None
        return np.zeros(n), np.zeros(n), draws, w, idx


def test_nu_selects_the_entry_point(monkeypatch):
    ctx = Ctx()
    monkeypatch.setattr(_lib, "default_context", lambda device=0: ctx)
    A, y, prior, folds = problem()
    plain = cv.kfold_cv(A, y, prior, folds, 10, seed=1, return_draws=True)
    assert ctx.calls[-1][0] == "gauss"
    assert set(plain) == {"elpd_cv", "se", "cv_rmse", "elpd_fold", "n_fold", "n_points", "n_folds", "n_draws",
                          "elpd_cv_i", "cv_mean_i", "seeds", "draws"}          # today's keys, no more
    t = cv.kfold_cv(A, y, prior, folds, 10, burn=2, thin=3, n_chains=2, seed=1, nu=4, return_draws=True,
                    return_row_weights=True)
    kind, kw = ctx.calls[-1]
    assert kind == "t" and kw["nu"] == 4.0 and kw["nu_grid"] is None
    assert t["likelihood"] == "student_t" and t["nu"] == 4.0 and "nu_draws" not in t
    assert t["draws"].shape == (4, 2, 3, 4) and t["row_weights"].shape == (4, 2, 40) and t["n_draws"] == 6
    assert t["seeds"].shape == (4, 2)
    e = cv.kfold_cv(A, y, prior, folds, 10, seed=1, nu="estimate", nu_grid=[1.0, 2.0, 8.0, 30.0],
                    nu_prior=[1.0, 1.0, 2.0, 0.0], nu_init=2.0, return_draws=True)
    kind, kw = ctx.calls[-1]
    assert kind == "t" and kw["nu"] is None and kw["nu_init"] == 1
    assert np.array_equal(kw["nu_grid"], [1.0, 2.0, 8.0, 30.0]) and np.array_equal(kw["nu_weight"], [1, 1, 2, 0])
    assert e["nu"] == 8.0 and e["nu_draws"].shape == (4, 1, 10) and (e["nu_draws"] == 8.0).all()
    assert "row_weights" not in e
    d = cv.kfold_cv(A, y, prior, folds, 10, seed=1, nu="estimate")
    grid, weight, init = robust_nu_prior()
    kind, kw = ctx.calls[-1]
    assert np.array_equal(kw["nu_grid"], grid) and np.array_equal(kw["nu_weight"], weight) and kw["nu_init"] == init
    assert "nu_draws" not in d and "draws" not in d and d["nu"] == grid[2]


def _bmc():
    import pandas as pd
    from pybmc_amd.bmc import BayesianModelCombination
    df = pd.DataFrame({"N": [1, 2, 3, 4], "Z": [1, 1, 2, 2], "a": [1.0, 2.0, 3.0, 4.0],
                       "b": [1.5, 2.5, 2.0, 3.0], "truth": [1.2, 2.2, 2.6, 3.3]})
    b = BayesianModelCombination(["a", "b"], {"p": df}, "truth")
    b.U_hat = np.ones((4, 1))
    b.Vt_hat = np.ones((1, 2))
    b.S_hat = np.ones(1)
    b.centered_experiment_train = np.array([0.1, -0.2, 0.3, 0.0])
    b._predictions_mean_train = np.array([1.0, 2.0, 3.0, 4.0])
    return b


def test_validate_dispatch(monkeypatch):
    seen = []

    def fake(A, y, prior, folds, iterations, **kw):
        seen.append((iterations, kw))
        return {"cv_mean_i": np.full(len(y), 0.5), "elpd_cv": -1.0}

    monkeypatch.setattr(cv, "kfold_cv", fake)
    b = _bmc()
    fresh = _bmc()
    fresh.U_hat = None
    for opts in (None, {"sampler": "student_t"}):
        with pytest.raises(ValueError, match="orthogonalize"):
            fresh.validate(training_options=opts)
    # options that name the Gaussian sampler, or nothing and no fit: the plain cross_validate() call
    for opts in (None, {"iterations": 30, "burn": 5}, {"sampler": "gibbs_sampling", "iterations": 30, "burn": 5}):
        seen.clear()
        out = b.validate(n_folds=2, training_options=opts, seed=3)
        want = b.cross_validate(n_folds=2, training_options=opts, seed=3)
        assert len(seen) == 2 and seen[0] == seen[1] and "nu" not in seen[0][1]
        assert set(out) == set(want) >= {"folds", "predicted", "truth", "residual"}
    # the t options: kfold_cv(nu=...), and cross_validate()'s extras
    seen.clear()
    out = b.validate(n_folds=2, training_options={"sampler": "student_t", "nu": 3, "iterations": 30, "burn": 5,
                                                  "thin": 2, "n_chains": 3}, seed=3)
    it, kw = seen[0]
    assert it == 30 and kw["nu"] == 3.0 and kw["burn"] == 5 and kw["thin"] == 2 and kw["n_chains"] == 3
    assert kw["seed"] == 3 and not any(key in kw for key in ("nu_grid", "nu_prior", "nu_init"))
    np.testing.assert_allclose(out["predicted"], 0.5 + b._predictions_mean_train)
    np.testing.assert_allclose(out["truth"], b.centered_experiment_train + b._predictions_mean_train)
    np.testing.assert_allclose(out["residual"], b.centered_experiment_train - 0.5)
    assert np.array_equal(out["folds"], cv.fold_labels(4, 2, 3)) and "groups" not in out
    b.validate(groups=np.array([7, 7, 9, 9]), training_options={"sampler": "student_t"})
    assert seen[-1][1]["nu"] == 4.0                                   # train()'s default
    b.validate(n_folds=2, training_options={"sampler": "student_t", "nu": "estimate", "nu_grid": [1.0, 5.0],
                                            "nu_init": 5.0})
    assert seen[-1][1]["nu"] == "estimate" and seen[-1][1]["nu_grid"] == [1.0, 5.0] and seen[-1][1]["nu_init"] == 5.0
    # no sampler named: the likelihood of the last train()
    b._trained_with = ("student_t", [np.zeros(1), np.eye(1), 1.0, 0.02], 2.5)
    b.validate(n_folds=2, training_options={"iterations": 30, "burn": 5})
    assert seen[-1][1]["nu"] == 2.5
    b._trained_with = ("student_t", [np.zeros(1), np.eye(1), 1.0, 0.02], "estimate")
    b._nu_prior = (np.array([1.0, 4.0]), np.array([0.5, 0.5]))
    b.validate(n_folds=2)
    assert seen[-1][1]["nu"] == "estimate" and np.array_equal(seen[-1][1]["nu_grid"], [1.0, 4.0])
    assert np.array_equal(seen[-1][1]["nu_prior"], [0.5, 0.5])
    b.validate(n_folds=2, training_options={"sampler": "gibbs_sampling"})   # the options win
    assert "nu" not in seen[-1][1]
    with pytest.raises(ValueError, match="simplex"):
        b.validate(training_options={"sampler": "simplex"})
    # cross_validate() and component_path() keep refusing
    for call in (b.cross_validate, b.component_path):
        with pytest.raises(ValueError, match="supports the Gaussian Gibbs sampler only"):
            call(n_folds=2)
        with pytest.raises(ValueError, match="supports the Gaussian Gibbs sampler only"):
            call(n_folds=2, training_options={"sampler": "student_t"})
