"""Time the component path in one call (``pybmc_amd.cv.cv_component_path``) next to the loop a user
writes without it: ``kfold_cv(A[:, :k], ...)`` once per candidate k.

Shapes: 629 x 3 (candidates 1 .. 3) and 10 000 x 32 (candidates 1 .. 32), F = 10 folds, C = 4 chains,
T = 50 000 iterations, the same seeds on both sides.  Host clock around each side (both return when
their results are on the host); the two alternate in one process, --reps timed rounds after --warmup
untimed ones.  One JSON line per shape: both medians, best times, the loop's own max - min spread (the
yardstick for "no slower than the loop") and whether the two agree bit for bit.
Usage: python scripts/cvpath_bench.py [--reps 5] [--shapes c1,c2] [--iters 50000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("c1", 629, 3), ("c2", 10000, 32))


def make_case(n, k, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, k)) / np.sqrt(n)
    beta = rng.standard_normal(k)
    sig = np.linalg.norm(X @ beta) / np.sqrt(n) / 10.0
    y = X @ beta + sig * rng.standard_normal(n)
    return X, y, [np.zeros(k), np.eye(k) * 10.0, 1.0, 0.02 * sig ** 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="c1,c2")
    ap.add_argument("--folds", type=int, default=10)
    ap.add_argument("--chains", type=int, default=4)
    ap.add_argument("--iters", type=int, default=50000)
    a = ap.parse_args()

    import torch
    from pybmc_amd import cv
    from pybmc_amd.chains import chain_seeds

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: cvpath_bench measures the device and has no CPU mode")
    F, C, T = a.folds, a.chains, a.iters
    for name, n, k in SHAPES:
        if name not in a.shapes.split(","):
            continue
        A, y, prior = make_case(n, k)
        b0, C0, nu0, s20 = prior
        folds = cv.fold_labels(n, F, seed=0)
        seeds = chain_seeds(1, np.arange(F * C)).reshape(F, C)
        cols = [np.ascontiguousarray(A[:, :j]) for j in range(1, k + 1)]

        def one_call():
            return cv.cv_component_path(A, y, prior, folds, T, n_chains=C, seeds=seeds)["elpd_cv_i"]

        def loop():
            return np.stack([cv.kfold_cv(cols[j - 1], y, [b0[:j], C0[:j, :j], nu0, s20], folds, T,
                                         n_chains=C, seeds=seeds)["elpd_cv_i"] for j in range(1, k + 1)])

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
        out = {"shape": name, "n": n, "k_max": k, "candidates": k, "folds": F, "chains": C, "iters": T,
               "call_ms_median": float(np.median(t_call)), "call_ms_best": min(t_call),
               "loop_ms_median": float(np.median(t_loop)), "loop_ms_best": min(t_loop),
               "loop_ms_spread": max(t_loop) - min(t_loop),
               "loop_over_call": float(np.median(t_loop) / np.median(t_call)),
               "same_bits": bool(np.array_equal(e_call, e_loop))}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
