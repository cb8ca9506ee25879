"""Time the Student-t Gibbs sampler with the degrees of freedom estimated (``bmc_robust_run_nu_device``,
robust_chain_kernel<KC, true>) next to the fixed-nu call (``bmc_robust_run_device``) on the same
problem, seeds and chain count.

Shapes: 629 x 3 (T = 50 000 sweeps) and 10 000 x 32 (T = 2 000), with 1, 64 and 256 chains.  Device
time: HIP events on the library's stream around one device-mode call writing device buffers (variate
fill, the pack kernel and the loop kernel; no copy of the samples).  The two calls alternate in one
process, --reps of each after --warmup of each; medians are reported: microseconds per sweep for all
chains of either call and their ratio.  The estimated-nu call uses the default grid and prior of
``gibbs_sampler_robust(nu="estimate")``.  One JSON line per (shape, chain count).
Usage: python scripts/robust_nu_bench.py [--reps 5] [--warmup 1] [--chains 1,64,256]
[--shapes reference_size,c2] [--quick]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SHAPES = [("reference_size", 629, 3, 50000), ("c2", 10000, 32, 2000)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chains", default="1,64,256")
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--quick", action="store_true", help="a tenth of the sweeps, 3 repetitions")
    a = ap.parse_args()

    import torch
    from pybmc_amd import _lib
    from pybmc_amd.inference_utils import robust_nu_prior
    from robust_bench import make_case

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: robust_nu_bench measures the device and has no CPU mode")
    dev = torch.device("cuda", 0)
    ctx = _lib.default_context(0)
    stream = torch.cuda.Stream(dev)
    ctx.set_stream(stream.cuda_stream)
    grid, weight, init = robust_nu_prior()
    for name, n, k, T in SHAPES:
        if name not in a.shapes.split(","):
            continue
        if a.quick:
            T, a.reps = T // 10, 3
        y, X, prior = make_case(n, k, 0)
        ctx.set_problem(y, X)
        ctx.set_prior(*prior)
        for C in (int(v) for v in a.chains.split(",")):
            seeds = np.arange(C, dtype=np.uint64) + 1
            out = torch.empty((C, T, k + 1), dtype=torch.float64, device=dev)
            w = torch.empty((C, n), dtype=torch.float64, device=dev)
            idx = torch.empty((C, T), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()

            def estimated():
                return ctx.robust_run_nu_device(grid, weight, init, C, T, 0, seeds, out.data_ptr(),
                                                idx.data_ptr(), w.data_ptr())

            def fixed():
                return ctx.robust_run_device(4.0, C, T, 0, seeds, out.data_ptr(), w.data_ptr())

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                st = fn()
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1), st["loop_ms"]

            for _ in range(a.warmup):
                estimated()
                fixed()
            t_e, t_f, l_e, l_f = [], [], [], []
            for _ in range(a.reps):
                ms, loop = timed(estimated)
                t_e.append(ms)
                l_e.append(loop)
                ms, loop = timed(fixed)
                t_f.append(ms)
                l_f.append(loop)
            nu_mean = float(torch.as_tensor(grid, device=dev)[idx.long()].mean())
            me, mf = float(np.median(t_e)), float(np.median(t_f))
            print(json.dumps({"shape": name, "n": n, "k": k, "n_chains": C, "sweeps": T,
                              "estimated_ms_median": me, "estimated_ms_all": t_e,
                              "fixed_ms_median": mf, "fixed_ms_all": t_f,
                              "estimated_loop_ms_median": float(np.median(l_e)),
                              "fixed_loop_ms_median": float(np.median(l_f)),
                              "estimated_us_per_sweep": 1e3 * me / T, "fixed_us_per_sweep": 1e3 * mf / T,
                              "estimated_over_fixed": me / mf, "mean_nu": nu_mean}), flush=True)
            del out, w, idx
    ctx.set_stream(None)


if __name__ == "__main__":
    main()
