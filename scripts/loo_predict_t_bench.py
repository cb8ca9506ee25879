"""Time the leave-one-out predictive moments under the Student-t likelihood next to their Gaussian
sibling and to PSIS-LOO on the same device arrays.

Shapes: C1 (377 x 3) and C2 (10 000 x 32), each with 50 000 draws: the inputs of
scripts/score_bench.py.  Device time: HIP events on the library's stream around one call of the
device entry point (all passes, the per-point fit and the copy of the result vectors).  Four calls
alternate in one process, medians of --reps rounds after --warmup rounds (the method of
scripts/tscore_bench.py): ``bmc_psis_loo_predict_t_device`` at --nu, ``bmc_psis_loo_predict_tv_device``
with nu cycling over the draws through 2.5 / 4 / 50, ``bmc_psis_loo_predict_device`` (Gaussian) and
``bmc_psis_loo_t_device`` at --nu.  With --other-lib PATH the Gaussian ``bmc_psis_loo_predict_device``
of another build of the library (the parent commit's, say) joins the same rounds on a context of its
own, so that the two builds alternate on one machine; the smallest and largest time of the
Gaussian call are printed with its median for that comparison.  One JSON line per shape.
Usage: python scripts/loo_predict_t_bench.py [--reps 5] [--nu 4] [--shapes c1,c2] [--other-lib PATH]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def alternating(stream, calls, warmup, reps):
    """Per call the times (ms) of `reps` rounds in which every call of `calls` runs once, in order."""
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
    return ms


def bind_other(path):
    """Another build of the library, which may lack the newest entry points: what it exports is bound."""
    from pybmc_amd import _lib
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
    for name, (res, args) in _lib.PROTOTYPES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nu", type=float, default=4.0)
    ap.add_argument("--shapes", default="c1,c2")
    ap.add_argument("--other-lib", default=None)
    a = ap.parse_args()

    import torch
    from score_bench import SHAPES, make_case
    from pybmc_amd import _lib

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: loo_predict_t_bench measures the device and has no CPU mode")
    dev = torch.device("cuda", 0)
    ctx = _lib.default_context(0)
    stream = torch.cuda.Stream(dev)
    ctx.set_stream(stream.cuda_stream)
    other = None
    if a.other_lib:
        other = _lib.Context(0, lib=bind_other(a.other_lib))
        other.set_stream(stream.cuda_stream)
    for name, n, k, S in SHAPES:
        if name not in a.shapes.split(","):
            continue
        A, y, th = make_case(n, k, S, 0)
        dA, dy, dth = (torch.as_tensor(v, device=dev) for v in (A, y, th))
        values = np.array([2.5, 4.0, 50.0])
        didx = torch.as_tensor((np.arange(S) % 3).astype(np.int32), device=dev)
        torch.cuda.synchronize()
        args = (dA.data_ptr(), n, k, k, _lib.BMC_ROW_MAJOR, dy.data_ptr(), dth.data_ptr(), S, k + 1)
        calls = [lambda: ctx.psis_loo_predict_t_device(*args, a.nu),
                 lambda: ctx.psis_loo_predict_tv_device(*args, values, didx.data_ptr()),
                 lambda: ctx.psis_loo_predict_device(*args),
                 lambda: ctx.psis_loo_t_device(*args, a.nu)]
        if other is not None:
            calls.append(lambda: other.psis_loo_predict_device(*args))
        ms = alternating(stream, calls, a.warmup, a.reps)
        med = [float(np.median(m)) for m in ms]
        out = {"shape": name, "n_points": n, "k": k, "n_draws": S, "nu": a.nu,
               "predict_t_ms": med[0], "predict_tv_ms": med[1], "predict_gauss_ms": med[2],
               "psis_loo_t_ms": med[3], "predict_t_over_gauss": med[0] / med[2],
               "predict_t_over_psis_loo_t": med[0] / med[3],
               "predict_gauss_ms_min_max": [float(min(ms[2])), float(max(ms[2]))]}
        if other is not None:
            out.update(other_predict_gauss_ms=med[4],
                       other_predict_gauss_ms_min_max=[float(min(ms[4])), float(max(ms[4]))])
        print(json.dumps(out), flush=True)
        del dA, dy, dth, didx
    ctx.set_stream(None)
    if other is not None:
        other.set_stream(None)


if __name__ == "__main__":
    main()
