"""Time the leave-one-out predictive moments (``pybmc_amd.scoring.psis_loo_predict``) next to
PSIS-LOO on the same device arrays.

Shapes: C1 (377 x 3, 50 000 draws) and C2 (10 000 x 32, 50 000 draws), the inputs of
scripts/loo_bench.py.  Device time: HIP events on the library's stream around one call of the
device entry point (all passes, the per-point fit and the copy of the result vectors), best and
median of --reps calls after --warmup calls, for ``bmc_psis_loo_device`` and
``bmc_psis_loo_predict_device`` in the same process.  The shares of the kernels are not measured
here: run this script under ``rocprofv3 --kernel-trace --stats -- python
scripts/loo_predict_bench.py`` for them.  One JSON line per shape.
Usage: python scripts/loo_predict_bench.py [--reps 9] [--shapes c1,c2]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shapes", default="c1,c2")
    a = ap.parse_args()

    import torch
    from loo_bench import timed
    from score_bench import SHAPES, make_case
    from pybmc_amd import _lib

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: loo_predict_bench measures the device and has no CPU mode")
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
        loo, l_best, l_med = timed(stream, lambda: ctx.psis_loo_device(*args), a.warmup, a.reps)
        got, p_best, p_med = timed(stream, lambda: ctx.psis_loo_predict_device(*args), a.warmup, a.reps)
        out = {"shape": name, "n_points": n, "k": k, "n_draws": S,
               "loo_ms_best": l_best, "loo_ms_median": l_med, "predict_ms_best": p_best,
               "predict_ms_median": p_med, "predict_over_loo": p_best / l_best,
               "same_elpd_bits": bool(np.array_equal(loo["elpd_loo"], got["elpd_loo"])),
               "loo_rmse": float(np.sqrt(np.mean((y - got["loo_mean"]) ** 2))),
               "min_ess": float(np.min(got["ess"]))}
        print(json.dumps(out), flush=True)
        del dA, dy, dth
    ctx.set_stream(None)


if __name__ == "__main__":
    main()
