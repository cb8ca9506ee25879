"""Time the posterior predictive check (``pybmc_amd.ppc``, kernels_ppc.hip) on device arrays, next
to the WAIC call on the same arrays.

Shapes: 629 x 3 with 50 000 draws, 10 000 x 32 with 50 000 draws and with 400 000 draws.  Device
time: HIP events on the library's stream around one call of the device entry point
(``bmc_ppc_device``: the two pad kernels, the tile kernel and the copy of the per-draw results;
``bmc_pointwise_loglik_device``: pad, constants, tile kernel, merge and its copies).  The two calls
alternate in one process, --reps of each after --warmup of each; medians are reported, their ratio,
and the PPC's elements (points x draws) per nanosecond.  The yardstick for the middle shape is the
predictive GEMM (``python bench.py --full``, ``predict_c5``), which forms as many elements with the
same noise.  One JSON line per shape.  Usage: python scripts/ppc_bench.py [--reps 5] [--warmup 2]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("reference_size", 629, 3, 50000), ("c2", 10000, 32, 50000), ("c2_8chains", 10000, 32, 400000)]


def make_case(n, k, S, seed):
    rng = np.random.default_rng(seed)
    A = np.linalg.qr(rng.standard_normal((n, k)))[0]
    b = rng.standard_normal(k)
    y = A @ b + 0.1 * rng.standard_normal(n)
    sig = 0.1 * (1 + rng.standard_normal(S) / np.sqrt(2 * n))
    return A, y, np.column_stack([A.T @ y + sig[:, None] * rng.standard_normal((S, k)), sig])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    a = ap.parse_args()

    import torch
    from pybmc_amd import _lib

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: ppc_bench measures the device and has no CPU mode")
    dev = torch.device("cuda", 0)
    ctx = _lib.default_context(0)
    stream = torch.cuda.Stream(dev)
    ctx.set_stream(stream.cuda_stream)
    for name, n, k, S in SHAPES:
        if name not in a.shapes.split(","):
            continue
        A, y, th = make_case(n, k, S, 0)
        dA, dy, dth = (torch.as_tensor(v, device=dev) for v in (A, y, th))
        center = float(np.mean(y))
        torch.cuda.synchronize()

        def ppc():
            return ctx.ppc_device(dA.data_ptr(), n, k, k, _lib.BMC_ROW_MAJOR, dy.data_ptr(),
                                  dth.data_ptr(), S, k + 1, None, 12345, center)

        def waic():
            return ctx.pointwise_loglik_device(dA.data_ptr(), n, k, k, _lib.BMC_ROW_MAJOR,
                                               dy.data_ptr(), dth.data_ptr(), S, k + 1)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            out = fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1), out

        for _ in range(a.warmup):
            ppc()
            waic()
        t_ppc, t_waic = [], []
        for _ in range(a.reps):
            ms, got = timed(ppc)
            t_ppc.append(ms)
            t_waic.append(timed(waic)[0])
        mp, mw = float(np.median(t_ppc)), float(np.median(t_waic))
        chi2_p = float(np.mean(got["t_rep"][:, 6] >= got["t_obs2"][:, 0]))
        print(json.dumps({"shape": name, "n_points": n, "k": k, "n_draws": S, "ppc_ms_median": mp,
                          "ppc_ms_all": t_ppc, "waic_ms_median": mw, "waic_ms_all": t_waic,
                          "ppc_over_waic": mp / mw, "elements_per_ns": n * S / mp / 1e6,
                          "workgroups": -(-S // 64), "p_chi2": chi2_p}), flush=True)
        del dA, dy, dth
    ctx.set_stream(None)


if __name__ == "__main__":
    main()
