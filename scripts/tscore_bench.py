"""Time the Student-t scoring calls next to their Gaussian siblings on the same device arrays.

Shapes: C1 (377 x 3) and C2 (10 000 x 32), each with 50 000 draws: the inputs of
scripts/score_bench.py.  Device time: HIP events on the library's stream around one call of the
device entry point; the Student-t call (nu = 4) and the Gaussian call alternate in one process,
medians of --reps pairs after --warmup pairs, for ``bmc_pointwise_loglik[_t]_device`` and for
``bmc_psis_loo[_t]_device``.  The two densities differ in the epilogue alone (one log1p per element
in place of a multiply-add), so the ratio t / Gaussian is the price of that logarithm where the
epilogue's vector instructions bound the call.  One JSON line per shape.
Usage: python scripts/tscore_bench.py [--reps 5] [--nu 4] [--shapes c1,c2]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def alternating(stream, calls, warmup, reps):
    """Medians (ms) of `reps` rounds in which every call of `calls` runs once, in order."""
    import torch
    for _ in range(warmup):
        for call in calls:
            call()
    ms = [[] for _ in calls]
    for _ in range(reps):
        for j, call in enumerate(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            ms[j].append(e0.elapsed_time(e1))
    return [float(np.median(m)) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nu", type=float, default=4.0)
    ap.add_argument("--shapes", default="c1,c2")
    a = ap.parse_args()

    import torch
    from score_bench import SHAPES, make_case
    from pybmc_amd import _lib

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: tscore_bench measures the device and has no CPU mode")
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
        pw_t, pw_g = alternating(stream, [lambda: ctx.pointwise_loglik_t_device(*args, a.nu),
                                          lambda: ctx.pointwise_loglik_device(*args)], a.warmup, a.reps)
        loo_t, loo_g = alternating(stream, [lambda: ctx.psis_loo_t_device(*args, a.nu),
                                            lambda: ctx.psis_loo_device(*args)], a.warmup, a.reps)
        print(json.dumps({"shape": name, "n_points": n, "k": k, "n_draws": S, "nu": a.nu,
                          "pointwise_t_ms": pw_t, "pointwise_gauss_ms": pw_g,
                          "pointwise_t_over_gauss": pw_t / pw_g, "psis_loo_t_ms": loo_t,
                          "psis_loo_gauss_ms": loo_g, "psis_loo_t_over_gauss": loo_t / loo_g}),
              flush=True)
        del dA, dy, dth
    ctx.set_stream(None)


if __name__ == "__main__":
    main()
