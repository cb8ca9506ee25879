"""The calls whose bits tests/test_basis_golden_gpu.py holds and scripts/record_basis_golden.py
records: what the prior-basis algebra (bmc_basis.h) decides, through the public entry points.

PRIOR_CASES    set_problem + set_prior on a CV.problem: basis() and conditional_moments(1.0), and
               (k <= 64) one default-rss and one rss="gram" gibbs_sampler chain;
CV_CASES       kfold_cv and cv_component_path under seed 5: draws, elpd_cv_i, cv_mean_i.
T = 40 everywhere.  Every golden file stays below 64 KB (the 65 x 65 matrices of the widest
problem go into a file each)."""
import os

import numpy as np

import cv_reference as CV

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "basis")
T = 40
SEED = 5

# name: ((n, k, snr, scale), chains recorded)
PRIOR_CASES = {
    "prior_150x3": ((150, 3, 10.0, 1.0), True),
    "prior_90x17_scaled": ((90, 17, 1e5, 1e3), True),
    "prior_200x65": ((200, 65, 10.0, 1.0), False),     # the branch without G, u0, g0
}


def balanced(n, F):
    return np.random.default_rng(n).permutation(np.arange(n) % F).astype(np.int64)


def cv_case(name):
    """(A, y, prior, folds, C, components): small and tight as in test_cvpath_gpu.py"""
    if name == "small":
        A, y, prior, _ = CV.problem(150, 3, 10.0)
        return A, y, prior, CV.unequal_folds(150, 5, 7), 2, (2, 3)
    if name == "tight":
        A, y, prior, _ = CV.problem(90, 17, 1e5, scale=1e3)
        return A, y, prior, balanced(90, 3), 1, (5, 17)
    if name == "width_edge":
        A, y, prior, _ = CV.problem(200, 33, 10.0)
        return A, y, prior, balanced(200, 2), 1, (32, 33)
    raise KeyError(name)


CV_CASES = ("small", "tight", "width_edge")


def golden_path(stem):
    return os.path.join(GOLDEN_DIR, stem + ".npz")


def run_prior_case(ctx, name):
    """{file stem: {key: array}} of one PRIOR_CASES entry on the context ``ctx``"""
    from pybmc_amd import gibbs_sampler

    (n, k, snr, scale), chains = PRIOR_CASES[name]
    A, y, prior, _ = CV.problem(n, k, snr, scale=scale)
    ctx.set_problem(y, A)
    ctx.set_prior(*prior)
    W, lam, s2 = ctx.basis()
    mean, cov = ctx.conditional_moments(1.0)
    out = {name + "_basis": {"W": W, "lam": lam, "sigma2_init": np.float64(s2)},
           name + "_moments": {"mean": mean, "cov": cov}}
    if chains:
        out[name + "_chains"] = {
            "data": gibbs_sampler(y, A, T, prior, seeds=[SEED]),
            "gram": gibbs_sampler(y, A, T, prior, seeds=[SEED], rss="gram")}
    return out


def run_cv_case(name):
    """{file stem: {key: array}} of one CV_CASES entry: the kfold_cv call on the whole design and
    the cv_component_path call on its components"""
    from pybmc_amd import cv

    A, y, prior, folds, C, comps = cv_case(name)
    one = cv.kfold_cv(A, y, prior, folds, T, n_chains=C, seed=SEED, return_draws=True)
    path = cv.cv_component_path(A, y, prior, folds, T, components=comps, n_chains=C, seed=SEED,
                                return_draws=True)
    out = {"kfold_" + name: {key: one[key] for key in ("draws", "elpd_cv_i", "cv_mean_i")},
           "path_" + name: {"elpd_cv_i": path["elpd_cv_i"], "cv_mean_i": path["cv_mean_i"]}}
    for j, kj in enumerate(comps):
        out["path_" + name][f"draws_{kj}"] = path["draws"][j]
    return out
