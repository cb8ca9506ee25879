"""Time exact K-fold cross-validation of a Student-t fit in one call (``pybmc_amd.cv.kfold_cv(nu=4)``)
next to the loop a user writes without it: per fold ``gibbs_sampler_robust(n_chains=4)`` on the
training subset, then ``pointwise_log_likelihood(nu=4)`` on the held-out rows.

Shapes (the robust sampler's own sizes): 629 x 3 at T = 50 000 sweeps and 10 000 x 32 at T = 2 000,
F = 10 folds, C = 4 chains, same seeds on both sides.  Host clock around each side (both return
when their results are on the host); the two alternate in one process, --reps timed rounds after
--warmup untimed ones: the method of cv_bench.py.  One JSON line per shape: both medians, best
times, the loop's own max - min spread and the largest |elpd_cv_i| difference between the two (the
chains are the same bits, so this is the scorer's).
Usage: python scripts/cv_t_bench.py [--reps 5] [--shapes c1,c2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("c1", 629, 3, 50000), ("c2", 10000, 32, 2000))
NU = 4.0


def make_case(n, k, seed=0):
    """cv_bench.py's problem with a twentieth of the rows moved by ten sigma."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, k)) / np.sqrt(n)
    beta = rng.standard_normal(k)
    sig = np.linalg.norm(X @ beta) / np.sqrt(n) / 10.0
    y = X @ beta + sig * rng.standard_normal(n)
    bad = rng.choice(n, size=n // 20, replace=False)
    y[bad] += 10.0 * sig * rng.choice([-1.0, 1.0], size=bad.size)
    return X, y, [np.zeros(k), np.eye(k) * 10.0, 1.0, 0.02 * sig ** 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="c1,c2")
    ap.add_argument("--folds", type=int, default=10)
    ap.add_argument("--chains", type=int, default=4)
    a = ap.parse_args()

    import torch
    from pybmc_amd import cv, gibbs_sampler_robust, pointwise_log_likelihood
    from pybmc_amd.chains import chain_seeds

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: cv_t_bench measures the device and has no CPU mode")
    F, C = a.folds, a.chains
    for name, n, k, T in SHAPES:
        if name not in a.shapes.split(","):
            continue
        A, y, prior = make_case(n, k)
        folds = cv.fold_labels(n, F, seed=0)
        seeds = chain_seeds(1, np.arange(F * C)).reshape(F, C)

        def one_call():
            return cv.kfold_cv(A, y, prior, folds, T, n_chains=C, seeds=seeds, nu=NU)["elpd_cv_i"]

        def loop():
            elpd = np.empty(n)
            for f in range(F):
                tr = folds != f
                s = gibbs_sampler_robust(y[tr], np.ascontiguousarray(A[tr]), T, prior, NU, n_chains=C,
                                         seeds=seeds[f])
                elpd[~tr] = pointwise_log_likelihood(np.ascontiguousarray(A[~tr]), y[~tr], s, nu=NU)["lppd"]
            return elpd

        t_call, t_loop = [], []
        for rep in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            e_call = one_call()
            t1 = time.perf_counter()
            e_loop = loop()
            t2 = time.perf_counter()
            if rep >= a.warmup:
                t_call.append((t1 - t0) * 1e3)
                t_loop.append((t2 - t1) * 1e3)
        out = {"shape": name, "n": n, "k": k, "folds": F, "chains": C, "iters": T, "nu": NU,
               "call_ms_median": float(np.median(t_call)), "call_ms_best": min(t_call),
               "loop_ms_median": float(np.median(t_loop)), "loop_ms_best": min(t_loop),
               "loop_ms_spread": max(t_loop) - min(t_loop),
               "loop_over_call": float(np.median(t_loop) / np.median(t_call)),
               "max_abs_elpd_diff": float(np.abs(e_call - e_loop).max())}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
