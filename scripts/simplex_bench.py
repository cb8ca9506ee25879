"""Time the simplex sampler's persistent kernels for 1, 8, 64 and 256 chains per call.

Shapes: the reference's own size (629 x 3, 4 models: one wave per chain), a four-wave shape
(2500 x 3, 4 models) and a workgroup-form shape (10 000 x 32, 66 models: more than a lane per
model, 32 workgroups per chain, 8 chains per launch).  Time: ``stats.loop_ms`` (HIP events around
the launches of one call) per iteration of burn + iterations, for ALL chains of the call; median,
min and max of --reps calls after one warm-up call.  Every call of a shape is made in the same
process, so the figures of a line are comparable.  One JSON line per shape.

    python scripts/simplex_bench.py [--reps 5] [--iters 50000] [--shapes ref,w4,wg] [--chains 1,8,64,256]

A/B of library builds (one chain, the builds alternating in one process, as scripts/ab.py does for
the Gibbs loop; other builds come from ``make -C pybmc_amd/csrc variant NAME=x``):

    python scripts/simplex_bench.py --ab pybmc_amd/libpybmc_amd.so .ab/lib_x.so
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pybmc_amd import _lib  # noqa: E402

SHAPES = {"ref": (629, 3, 4), "w4": (2500, 3, 4), "wg": (10000, 32, 66)}   # rows, kept components, models
BURN, STEPSIZE = 1000, 0.001
VARIATE_DOUBLES = 2.5e8     # cap on chains x iterations x k (2 GB of proposal innovations)


def problem(n, k, km):
    rng = np.random.default_rng(n + k)
    A = rng.standard_normal((n, km))
    truth = A @ np.full(km, 1.0 / km) + 0.05 * rng.standard_normal(n)
    U, S, Vt = np.linalg.svd(A - A.mean(1, keepdims=True), full_matrices=False)
    S_hat = S[:k]
    return truth - A.mean(1), np.asfortranarray(U[:, :k]), Vt[:k] / S_hat[:, None], S_hat


def summary(us):
    us = np.asarray(us)
    return {"median": float(np.median(us)), "min": float(us.min()), "max": float(us.max()),
            "runs": [round(float(u), 4) for u in us]}


def scaling(a):
    ctx = _lib.Context(0)
    for name in a.shapes.split(","):
        n, k, km = SHAPES[name]
        y, X, Vt_hat, S_hat = problem(n, k, km)
        ctx.set_problem(y, X)
        out = {"shape": name, "n": n, "k": k, "n_models": km, "burn": BURN, "us_per_iteration": {}}
        for C in [int(c) for c in a.chains.split(",")]:
            iters = int(min(a.iters, VARIATE_DOUBLES // (C * k) - BURN))
            seeds = np.arange(C) + 1
            us, st = [], None
            for r in range(a.reps + 1):     # (the first call is the warm-up)
                _, acc, used, st = ctx.simplex_run_chains(Vt_hat, S_hat, C, iters, 1.0, 0.02, BURN, STEPSIZE,
                                                          seeds=seeds, return_stats=True)
                if r:
                    us.append(st["loop_ms"] * 1e3 / (iters + BURN))
            out["us_per_iteration"][str(C)] = dict(
                summary(us), iterations=iters, launches=st["launches"], groups_per_chain=st["groups_per_chain"],
                waves_per_group=st["waves_per_group"], acceptance=float(acc.mean() / iters))
        out["kernels"] = sorted(set(ctx.last_kernels()))
        print(json.dumps(out), flush=True)
    ctx.close()


def ab(a):
    _lib._share_hip_runtime_with_torch()
    libs = [(p, _lib.bind(os.path.abspath(p), mode=ctypes.RTLD_LOCAL)) for p in a.ab]
    for name in a.shapes.split(","):
        n, k, km = SHAPES[name]
        y, X, Vt_hat, S_hat = problem(n, k, km)
        ctxs = []
        for p, lib in libs:
            c = _lib.Context(0, lib=lib)
            c.set_problem(y, X)
            ctxs.append((p, c))
        times = {p: [] for p, _ in ctxs}
        first, same = None, True
        for r in range(a.reps + 1):         # (round 0 is the warm-up)
            order = ctxs[r % len(ctxs):] + ctxs[:r % len(ctxs)]
            for p, c in order:
                res, acc, used, st = c.simplex_run(Vt_hat, S_hat, a.iters, 1.0, 0.02, BURN, STEPSIZE, seed=3,
                                                   return_stats=True)
                if r:
                    times[p].append(st["loop_ms"] * 1e3 / (a.iters + BURN))
                if first is None:
                    first = res
                elif not np.array_equal(res, first):
                    same = False
                    print(f"NOTE {name}: {p} differs from the first build by {np.abs(res - first).max():.3e}",
                          flush=True)
        print(json.dumps({"shape": name, "n": n, "k": k, "n_models": km, "iterations": a.iters, "burn": BURN,
                          "chains": 1, "us_per_iteration": {p: summary(t) for p, t in times.items()},
                          "same_bits": same}), flush=True)
        for _, c in ctxs:
            c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50000)
    ap.add_argument("--shapes", default="ref,w4,wg")
    ap.add_argument("--chains", default="1,8,64,256")
    ap.add_argument("--ab", nargs="+", metavar="LIB", help="time one chain on each of these builds in turn")
    a = ap.parse_args()
    (ab if a.ab else scaling)(a)


if __name__ == "__main__":
    main()
