"""Time the PSIS-LOO kernels (``pybmc_amd.scoring.psis_loo``) next to WAIC on the same device arrays.

Shapes: C1 (377 x 3, 50 000 draws), C2 (10 000 x 32, 50 000 draws) and C2 with 8 pooled chains
(400 000 draws), the inputs of scripts/score_bench.py.  Device time: HIP events on the library's
stream around one call of the device entry point (all passes, the per-point fit and the copy of
the result vectors), best and median of --reps calls after --warmup calls, for
``bmc_pointwise_loglik_device`` (WAIC) and ``bmc_psis_loo_device`` in the same process.  The plan
(tail M, candidate cap, passes over the matrix that are launched) is printed with each line; the
share of each kernel is not measured here: run this script under
``rocprofv3 --kernel-trace --stats -- python scripts/loo_bench.py --no-reference`` for the
per-kernel times (loo_select_kernel launches after the last one that finds unsettled points
return at once).  One JSON line per shape.
Usage: python scripts/loo_bench.py [--reps 7] [--no-reference] [--shapes c1,c2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def timed(stream, call, warmup, reps):
    import torch
    for _ in range(warmup):
        got = call()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        got = call()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return got, min(ms), float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--shapes", default="c1,c2,c2_8chains")
    a = ap.parse_args()

    import torch
    from score_bench import SHAPES, make_case
    from pybmc_amd import _lib

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: loo_bench measures the device and has no CPU mode")
    dev = torch.device("cuda", 0)
    ctx = _lib.default_context(0)
    stream = torch.cuda.Stream(dev)
    ctx.set_stream(stream.cuda_stream)
    for name, n, k, S in SHAPES:
        if name not in a.shapes.split(","):
            continue
        A, y, th = make_case(n, k, S, 0)
        dA, dy, dth = (torch.as_tensor(v, device=dev) for v in (A, y, th))
        torch.cuda.synchronize()
        args = (dA.data_ptr(), n, k, k, _lib.BMC_ROW_MAJOR, dy.data_ptr(), dth.data_ptr(), S, k + 1)
        _, w_best, w_med = timed(stream, lambda: ctx.pointwise_loglik_device(*args), a.warmup, a.reps)
        got, l_best, l_med = timed(stream, lambda: ctx.psis_loo_device(*args), a.warmup, a.reps)
        M = min(S // 5, int(np.ceil(3 * np.sqrt(S))))
        cap = 64
        while cap < 2 * (M + 1):
            cap *= 2
        out = {"shape": name, "n_points": n, "k": k, "n_draws": S, "tail": M, "cap": cap,
               "waic_ms_best": w_best, "waic_ms_median": w_med, "loo_ms_best": l_best,
               "loo_ms_median": l_med, "loo_over_waic": l_best / w_best,
               "pareto_k_max": float(np.max(got["pareto_k"])),
               "elpd_loo": float(np.sum(got["elpd_loo"]))}
        if not a.no_reference and name == "c1":
            import psis_reference as P
            t0 = time.perf_counter()
            ref = P.pointwise(A, y, th)
            out["numpy_reference_s"] = time.perf_counter() - t0
            out["max_err"] = {
                "elpd_loo": float(np.max(np.abs(got["elpd_loo"] - ref["elpd_loo"])
                                         / np.maximum(1, np.abs(ref["elpd_loo"])))),
                "pareto_k": float(np.max(np.abs(got["pareto_k"] - ref["pareto_k"])))}
        print(json.dumps(out), flush=True)
        del dA, dy, dth
    ctx.set_stream(None)


if __name__ == "__main__":
    main()
