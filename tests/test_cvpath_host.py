"""Host side of the component path (pybmc_amd.cv.path_summary, the argument checks of
cv_component_path and BayesianModelCombination.component_path): no GPU."""
import numpy as np
import pytest

import pybmc_amd
from pybmc_amd import _lib, cv


def test_exports():
    assert pybmc_amd.cv_component_path is cv.cv_component_path
    assert pybmc_amd.path_summary is cv.path_summary
    assert hasattr(pybmc_amd.BayesianModelCombination, "component_path")


def se_diff(a, b):
    """sqrt(n var_i(a_i - b_i, ddof=1)), written out"""
    d = np.asarray(a, dtype=float) - np.asarray(b, dtype=float)
    n = len(d)
    return np.sqrt(n * ((d - d.sum() / n) ** 2).sum() / (n - 1))


def test_path_summary_picks_the_best_and_its_differences():
    e = np.array([[-3.0, -2.0, -4.0, -1.0],     # -10
                  [-1.0, -1.5, -2.0, -0.5],     # -5: the best
                  [-1.0, -2.5, -2.0, -0.5],     # -6
                  [-2.0, -2.0, -2.0, -2.0]])    # -8
    s = cv.path_summary([2, 3, 5, 8], e)
    assert s["k_best"] == 3
    assert np.array_equal(s["elpd_diff"], [5.0, 0.0, 1.0, 3.0])
    want = [se_diff(e[1], e[0]), 0.0, se_diff(e[1], e[2]), se_diff(e[1], e[3])]
    assert s["se_diff"] == pytest.approx(want, rel=1e-15) and s["se_diff"][1] == 0.0
    # candidate 2 lies 5 behind with se_diff 2.58: outside; nothing smaller than the best is inside
    assert want[0] == pytest.approx(np.sqrt(4 * np.var(e[1] - e[0], ddof=1)), rel=1e-15)
    assert s["k_1se"] == 3


def test_a_tie_resolves_to_the_smallest_candidate():
    e = np.array([[-1.0, -2.0, -3.0], [-3.0, -2.0, -1.0], [-2.0, -2.0, -2.5]])
    s = cv.path_summary([1, 2, 3], e)
    assert s["k_best"] == 1 and s["k_1se"] == 1      # the best is also the smallest
    assert np.array_equal(s["elpd_diff"], [0.0, 0.0, 0.5])
    assert s["se_diff"][0] == 0.0 and s["se_diff"][1] == pytest.approx(se_diff(e[0], e[1]))


def test_one_standard_error_rule_includes_a_candidate_exactly_at_one_se():
    # elpd_diff == se_diff exactly: d = (0, 0, 0, 4) has sum 4 and sqrt(4 var(d, ddof=1)) = 4
    best = np.array([-1.0, -1.0, -1.0, -1.0])
    d = np.array([0.0, 0.0, 0.0, 4.0])
    assert se_diff(d, 0 * d) == 4.0 and d.sum() == 4.0
    e = np.array([best - d - 3.0, best - d, best])
    s = cv.path_summary([1, 2, 3], e)
    assert s["k_best"] == 3
    assert s["elpd_diff"][1] == s["se_diff"][1] == 4.0
    assert s["elpd_diff"][0] == 16.0 and s["se_diff"][0] == 4.0     # a constant shift adds no spread
    assert s["k_1se"] == 2                                          # exactly at one se: inside
    # a hair further out and it is the best alone
    e[1, 0] -= 1e-9
    assert cv.path_summary([1, 2, 3], e)["k_1se"] == 3
    with pytest.raises(ValueError):
        cv.path_summary([1, 2], e)


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
        return cv.cv_component_path(A, y, prior, folds, iterations, **kw)

    for bad, what in (((2, 1), "increasing"), ((1, 1, 2), "increasing"), ((0, 1), r"1 \.\. 3"),
                      ((1, 4), r"1 \.\. 3"), ((), "at least one"), ((True, 2), "integers"),
                      ((1.0, 2.0), "integers"), (np.array([1.0, 2.0]), "integers"), (2, "sequence")):
        with pytest.raises(ValueError, match=what):
            call(components=bad)
    wide = rng.standard_normal((200, 65))
    with pytest.raises(ValueError, match="at most 64"):
        call(A=wide, y=rng.standard_normal(200), prior=[np.zeros(65), np.eye(65), 1.0, 0.02],
             folds=np.arange(200) % 2)
    # a fold whose training set is smaller than the LARGEST candidate: 2 rows are enough for (1, 2)
    short = np.array([0] * (n - 2) + [1, 1])
    with pytest.raises(ValueError, match="fold 0: its training set has 2 rows, fewer than k = 3"):
        call(folds=short)
    with pytest.raises(AssertionError, match="a context was asked for"):
        call(folds=short, components=(1, 2))        # (valid: it gets as far as the device)
    with pytest.raises(ValueError, match="prior_info"):
        call(prior=[np.zeros(k), np.eye(k - 1), 1.0, 0.02])
    with pytest.raises(ValueError, match="prior_info"):
        call(prior=[np.zeros(2), np.eye(2), 1.0, 0.02], components=(1, 2))   # the prior is k_max wide
    with pytest.raises(ValueError, match="not both"):
        call(seed=1, seeds=np.ones((4, 1), dtype=np.uint64))
    with pytest.raises(ValueError, match="seeds must be"):
        call(seeds=np.ones((3, 4, 1), dtype=np.uint64))     # not per candidate: shared by all
    with pytest.raises(ValueError, match="seeds must be"):
        call(seeds=np.ones(4, dtype=np.uint64), n_chains=2)
    # and what kfold_cv refuses
    with pytest.raises(ValueError, match="integer"):
        call(folds=folds.astype(float))
    with pytest.raises(ValueError, match="fold 2 is empty"):
        call(folds=np.where(folds == 2, 0, folds))
    with pytest.raises(ValueError, match="float64"):
        call(A=A.astype(np.float32))
    with pytest.raises(ValueError, match="at least 2 draws"):
        call(iterations=10, burn=9)
    with pytest.raises(ValueError, match="y must be"):
        call(y=y[:-1])


def test_component_path_refuses_what_cross_validate_refuses(no_device):
    import pandas as pd
    rng = np.random.default_rng(2)
    df = pd.DataFrame(rng.standard_normal((30, 3)), columns=["m0", "m1", "m2"])
    df["truth"] = rng.standard_normal(30)
    df["Z"] = np.arange(30) % 5
    bmc = pybmc_amd.BayesianModelCombination(["m0", "m1", "m2"], {"p": df}, "truth")
    with pytest.raises(ValueError, match="orthogonalize"):
        bmc.component_path()
    bmc.orthogonalize("p", df, 2, method="svd")
    with pytest.raises(ValueError, match="simplex"):
        bmc.component_path(training_options={"sampler": "simplex"})
    with pytest.raises(ValueError, match="no column"):
        bmc.component_path(groups="N")
    with pytest.raises(ValueError, match="one entry per training row"):
        bmc.component_path(groups=np.arange(29))
    with pytest.raises(ValueError, match=r"1 \.\. 2"):
        bmc.component_path(components=(1, 3))
    assert "components_kept" in bmc.component_path.__doc__ and "k_1se" in bmc.component_path.__doc__
