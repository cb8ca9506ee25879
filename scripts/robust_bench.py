"""Time the Student-t (outlier-robust) Gibbs sampler (``bmc_robust_run_device``, kernels_robust.hip)
next to the Gaussian sampler (``bmc_gibbs_run_device``) on the same problem and chain count.

Shapes: 629 x 3 and 10 000 x 32, T sweeps (default 50 000), with 1, 64 and 256 chains.  Device time:
HIP events on the library's stream around one device-mode call writing a device buffer (variate
fill, the pack kernel and the loop kernels; no copy of the samples).  The two calls alternate in
one process, --reps of each after --warmup of each; medians are reported: microseconds per sweep for
all chains, the ratio to the Gaussian sampler, and the achieved f64 flop/s of the weighted Gram at
N k (k + 1) + 4 N k flops per sweep and chain.  One JSON line per (shape, chain count).  There is no
target: the feature has no predecessor.  Usage: python scripts/robust_bench.py [--iters 50000]
[--reps 5] [--warmup 1] [--chains 1,64,256] [--shapes reference_size,c2] [--quick]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("reference_size", 629, 3), ("c2", 10000, 32)]


def make_case(n, k, seed):
    rng = np.random.default_rng(seed)
    X = np.linalg.qr(rng.standard_normal((n, k)))[0]
    y = X @ (3 * rng.standard_normal(k)) + 0.1 * rng.standard_normal(n)
    bad = rng.choice(n, max(1, n // 20), replace=False)
    y[bad] += 0.8 * np.where(rng.random(len(bad)) < 0.5, -1, 1) * (1 + rng.random(len(bad)))
    return y, X, (np.zeros(k), np.eye(k), 1.0, 0.02)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chains", default="1,64,256")
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--quick", action="store_true", help="2 000 sweeps, 3 repetitions")
    a = ap.parse_args()
    if a.quick:
        a.iters, a.reps = 2000, 3

    import torch
    from pybmc_amd import _lib

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: robust_bench measures the device and has no CPU mode")
    dev = torch.device("cuda", 0)
    ctx = _lib.default_context(0)
    stream = torch.cuda.Stream(dev)
    ctx.set_stream(stream.cuda_stream)
    T = a.iters
    for name, n, k in SHAPES:
        if name not in a.shapes.split(","):
            continue
        y, X, prior = make_case(n, k, 0)
        ctx.set_problem(y, X)
        ctx.set_prior(*prior)
        for C in (int(v) for v in a.chains.split(",")):
            seeds = np.arange(C, dtype=np.uint64) + 1
            out = torch.empty((C, T, k + 1), dtype=torch.float64, device=dev)
            w = torch.empty((C, n), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()

            def robust():
                return ctx.robust_run_device(4.0, C, T, 0, seeds, out.data_ptr(), w.data_ptr())

            def gauss():
                return ctx.gibbs_run_device(C, T, seeds, out.data_ptr())

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                st = fn()
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1), st

            for _ in range(a.warmup):
                robust()
                gauss()
            t_r, t_g, loop = [], [], []
            for _ in range(a.reps):
                ms, st = timed(robust)
                t_r.append(ms)
                loop.append(st["loop_ms"])
                t_g.append(timed(gauss)[0])
            mr, mg, ml = float(np.median(t_r)), float(np.median(t_g)), float(np.median(loop))
            flops = (n * k * (k + 1) + 4 * n * k) * float(T) * C
            print(json.dumps({"shape": name, "n": n, "k": k, "n_chains": C, "sweeps": T,
                              "robust_ms_median": mr, "robust_ms_all": t_r, "robust_loop_ms_median": ml,
                              "gibbs_ms_median": mg, "gibbs_ms_all": t_g,
                              "robust_us_per_sweep": 1e3 * mr / T, "gibbs_us_per_sweep": 1e3 * mg / T,
                              "robust_over_gibbs": mr / mg, "gram_f64_tflops": flops / (ml * 1e-3) / 1e12,
                              "mean_row_weight": float(w.mean())}), flush=True)
            del out, w
    ctx.set_stream(None)


if __name__ == "__main__":
    main()
