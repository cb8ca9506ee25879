"""Time ``rank_diagnostics`` on a device array of the headline size, (64 chains, 50 000 draws,
33 columns) f64 = 845 MB, next to ``chain_diagnostics`` on the same data in the same process.

The data are scripts/diag_bench.py's: iid, AR(1) phi = 0.9 and AR(1) phi = 0.99 columns in turn.
The two calls alternate, --reps rounds after --warmup rounds.  Per call: the host clock around it
(both end in a stream synchronise), and for ``rank_diagnostics`` the library's own HIP events on its
stream (bmc_rank_last_timing): the sorts (gather and fold included), the rank / quantile / indicator
kernels, the classic leg on the derived series, the mean / sd pass.  Reports best and median of each
and the ratio of the medians.  Prints one JSON line.
Usage: python scripts/rank_diag_bench.py [--chains 64 --iters 50000 --cols 33 --cols-per-batch 0]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=64)
    ap.add_argument("--iters", type=int, default=50000)
    ap.add_argument("--cols", type=int, default=33)
    ap.add_argument("--burn", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cols-per-batch", type=int, default=0)
    a = ap.parse_args()

    import torch
    from diag_bench import make_data
    from pybmc_amd import _lib, chain_diagnostics, rank_diagnostics

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: rank_diag_bench measures the device and has no CPU mode")
    x = make_data(a.chains, a.iters, a.cols, 0)
    dx = torch.as_tensor(x, device="cuda:0")
    torch.cuda.synchronize()
    ctx = _lib.default_context(0)
    rank_t, classic_t, parts = [], [], []
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        classic = chain_diagnostics(dx, burn=a.burn)
        t1 = time.perf_counter()
        got = rank_diagnostics(dx, burn=a.burn, cols_per_batch=a.cols_per_batch)
        t2 = time.perf_counter()
        if r >= a.warmup:
            classic_t.append(1e3 * (t1 - t0))
            rank_t.append(1e3 * (t2 - t1))
            parts.append(ctx.rank_last_timing())
    med = lambda v: float(np.median(v))
    out = {
        "shape": [a.chains, a.iters, a.cols],
        "bytes": int(x.nbytes),
        "cols_per_batch": a.cols_per_batch,
        "rank_ms_best": min(rank_t), "rank_ms_median": med(rank_t),
        "chain_ms_best": min(classic_t), "chain_ms_median": med(classic_t),
        "ratio_median": med(rank_t) / med(classic_t),
        "split_ms_median": {k: med([p[k] for p in parts]) for k in parts[0]},
        "mean_sd_bit_equal": bool(np.array_equal(got["mean"], classic["mean"])
                                  and np.array_equal(got["sd"], classic["sd"])),
        "r_hat_max": float(np.nanmax(got["r_hat"])),
        "ess_bulk_min": float(np.nanmin(got["ess_bulk"])),
        "ess_tail_min": float(np.nanmin(got["ess_tail"])),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
