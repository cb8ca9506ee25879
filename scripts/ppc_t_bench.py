"""Time the posterior predictive check with Student-t replicated noise (``bmc_ppc_t_device``,
``bmc_ppc_tv_device``; kernels_ppc.hip) on device arrays, next to the Gaussian check
(``bmc_ppc_device``) on the same arrays.

Shapes: 629 x 3 and 10 000 x 32, both with 50 000 draws; for ``nu = 4`` and for a ``nu`` per draw
(64 distinct values between 1.5 and 50, the index on the device).  Device time: HIP events on the
library's stream around one call of the device entry point (the pad kernels, the tile kernel and
the copy of the per-draw results).  The three calls alternate in one process, --reps of each after
--warmup of each; medians are reported and the ratios of the two t forms to the Gaussian check.
One JSON line per shape.  Usage: python scripts/ppc_t_bench.py [--reps 5] [--warmup 2]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.ppc_bench import make_case  # noqa: E402

SHAPES = [("reference_size", 629, 3, 50000), ("c2", 10000, 32, 50000)]
NU = 4.0
NU_VALUES = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    a = ap.parse_args()

    import torch
    from pybmc_amd import _lib

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: ppc_t_bench measures the device and has no CPU mode")
    dev = torch.device("cuda", 0)
    ctx = _lib.default_context(0)
    stream = torch.cuda.Stream(dev)
    ctx.set_stream(stream.cuda_stream)
    for name, n, k, S in SHAPES:
        if name not in a.shapes.split(","):
            continue
        A, y, th = make_case(n, k, S, 0)
        dA, dy, dth = (torch.as_tensor(v, device=dev) for v in (A, y, th))
        values = np.geomspace(1.5, 50.0, NU_VALUES)
        index = np.random.default_rng(1).integers(0, NU_VALUES, S).astype(np.int32)
        didx = torch.as_tensor(index, device=dev)
        torch.cuda.synchronize()
        common = (dA.data_ptr(), n, k, k, _lib.BMC_ROW_MAJOR, dy.data_ptr(), dth.data_ptr(), S, k + 1, None, 12345)

        calls = {"gauss": lambda: ctx.ppc_device(*common, 0.0),
                 "t": lambda: ctx.ppc_t_device(*common, NU),
                 "tv": lambda: ctx.ppc_tv_device(*common, values, didx.data_ptr())}

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            out = fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1), out

        for _ in range(a.warmup):
            for fn in calls.values():
                fn()
        ms = {key: [] for key in calls}
        got = {}
        for _ in range(a.reps):
            for key, fn in calls.items():
                t, got[key] = timed(fn)
                ms[key].append(t)
        med = {key: float(np.median(v)) for key, v in ms.items()}
        print(json.dumps({"shape": name, "n_points": n, "k": k, "n_draws": S, "nu": NU,
                          "nu_values": NU_VALUES, "gauss_ms_median": med["gauss"], "t_ms_median": med["t"],
                          "tv_ms_median": med["tv"], "gauss_ms_all": ms["gauss"], "t_ms_all": ms["t"],
                          "tv_ms_all": ms["tv"], "t_over_gauss": med["t"] / med["gauss"],
                          "tv_over_gauss": med["tv"] / med["gauss"],
                          "t_elements_per_ns": n * S / med["t"] / 1e6, "workgroups": -(-S // 64),
                          "p_chi2": {key: float(np.mean(v["t_rep"][:, 6] >= v["t_obs2"][:, 0]))
                                     for key, v in got.items()}}), flush=True)
        del dA, dy, dth, didx
    ctx.set_stream(None)


if __name__ == "__main__":
    main()
