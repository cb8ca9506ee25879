"""Numpy reference of pybmc_amd.cv and the seeded cases its tests share (no GPU).

Per fold the posterior's one-off quantities are ``oracle.bmc_oracle.chain_setup`` on the training
subset, and the held-out rows are scored against that fold's draws by ``score_reference``.  The
training statistics by total-minus-own -- what the device path computes in one pass -- are restated
here in extended precision so that they can be held against the subset's own."""
import numpy as np

import score_reference as R
from oracle import bmc_oracle as O

# name: (n, k, folds, chains, signal-to-noise); the shapes of the issue's table
CASES = {
    "unequal": (150, 3, 5, 2, 10.0),     # unequal folds, one of a single row
    "one_col": (700, 1, 7, 1, 10.0),
    "tight": (90, 17, 3, 1, 1e6),        # rss0 is 1e-12 of |y|^2: must not cancel
    "wide": (1300, 64, 2, 1, 10.0),      # the last kernel width, half the data held out
    # the tight fit again with the data scaled by 1e3, so that sigma^2 (1e-4) is above the sampler's
    # 1e-6 floor and every draw depends on rss, itself 1e-10 of |y|^2
    "tight_scaled": (90, 17, 3, 1, 1e5),
}
SCALE = {"tight_scaled": 1e3}
T = 300


def problem(n, k, snr, scale=1.0):
    """(A, y, prior, sigma): the generator of test_gram_mode_gpu.py::test_same_chain_as_the_data_pass,
    the targets (signal and noise) multiplied by ``scale`` and the prior covariance by its square:
    the same problem in other units.  (With the covariance left at 10 I the coefficients, about
    1e3, lie 300 prior standard deviations from the prior mean and the posterior has a second mode
    at a large sigma, where prior and data trade places: nothing to hold a mean of sigma against.)"""
    rng = np.random.default_rng(n + k)
    X = rng.standard_normal((n, k)) / np.sqrt(n)
    beta = rng.standard_normal(k)
    sig = scale * np.linalg.norm(X @ beta) / np.sqrt(n) / snr
    y = scale * (X @ beta) + sig * rng.standard_normal(n)
    return X, y, [np.zeros(k), np.eye(k) * 10.0 * scale ** 2, 1.0, 0.02 * sig ** 2], sig


def unequal_folds(n, F, seed):
    """Labels 0 .. F-1 in random order with fold sizes 1, then growing: fold 0 holds ONE row."""
    w = np.arange(F, dtype=float)
    sizes = np.floor((n - 1) * w / w.sum()).astype(int)
    sizes[0] = 1
    sizes[-1] += n - sizes.sum()
    lab = np.repeat(np.arange(F), sizes)
    return np.random.default_rng(seed).permutation(lab).astype(np.int64)


def case(name):
    """(A, y, prior, folds, F, C) of a named case."""
    n, k, F, C, snr = CASES[name]
    A, y, prior, _ = problem(n, k, snr, SCALE.get(name, 1.0))
    if name == "unequal":
        folds = unequal_folds(n, F, 7)
    else:
        folds = np.random.default_rng(n).permutation(np.arange(n) % F).astype(np.int64)
    return A, y, prior, folds, F, C


def fold_statistics(A, y, folds, F):
    """(XtX [F, k, k], Xty [F, k]) of every fold's TRAINING rows as total minus own: the Gram of
    [A y] per fold, the folds added in ascending order, in extended precision."""
    Z = np.column_stack([A, y]).astype(np.longdouble)
    own = np.stack([Z[folds == f].T @ Z[folds == f] for f in range(F)])
    total = np.zeros_like(own[0])
    for f in range(F):
        total = total + own[f]
    train = (total[None] - own).astype(np.float64)
    return train[:, :-1, :-1], train[:, :-1, -1]


def subset_setup(A, y, prior, folds, f):
    tr = folds != f
    return O.chain_setup(y[tr], np.ascontiguousarray(A[tr]), prior)


def cv_reference(A, y, folds, F, draws):
    """elpd_cv_i and cv_mean_i of every row from the draws (F, C, kept, k+1) of its own fold."""
    n = len(y)
    elpd, mean = np.empty(n), np.empty(n)
    for f in range(F):
        held = folds == f
        th = draws[f].reshape(-1, draws.shape[-1])
        elpd[held] = R.pointwise(A[held], y[held], th)["lppd"]
        mean[held] = A[held] @ th[:, :-1].mean(axis=0)
    return elpd, mean


def summary(y, folds, F, elpd, mean):
    return {"elpd_cv": float(elpd.sum()), "se": R._se(elpd),
            "cv_rmse": float(np.sqrt(np.mean((y - mean) ** 2))),
            "elpd_fold": np.array([elpd[folds == f].sum() for f in range(F)]),
            "n_fold": np.array([int((folds == f).sum()) for f in range(F)])}
