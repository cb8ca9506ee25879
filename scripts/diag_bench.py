"""Time ``chain_diagnostics`` on a device array of the headline size, (64 chains, 50 000 draws,
33 columns) f64 = 845 MB, against the numpy FFT reference of the tests on the same data.

The columns mix iid draws, AR(1) with phi = 0.9 and AR(1) with phi = 0.99 (a column the scan
follows past the first lag block).  Device time: host clock around the whole call (it ends in a
stream synchronise: moments pass, every lag block, the host scan), best and median of --reps
calls after --warmup calls.  Reference time: one call of tests/diag_reference.diagnostics.
Prints one JSON line.  Usage: python scripts/diag_bench.py [--chains 64 --iters 50000 --cols 33]
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


def make_data(C, T, P, seed):
    rng = np.random.default_rng(seed)
    phi = np.array([(0.0, 0.9, 0.99)[j % 3] for j in range(P)])
    s = np.sqrt(1.0 - phi * phi)
    x = np.empty((C, T, P))
    x[:, 0] = rng.standard_normal((C, P))
    for t in range(1, T):
        x[:, t] = phi * x[:, t - 1] + s * rng.standard_normal((C, P))
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=64)
    ap.add_argument("--iters", type=int, default=50000)
    ap.add_argument("--cols", type=int, default=33)
    ap.add_argument("--burn", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-reference", action="store_true")
    a = ap.parse_args()

    import torch
    import diag_reference as R
    from pybmc_amd import chain_diagnostics
    from pybmc_amd.diagnostics import lag_blocks

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: diag_bench measures the device and has no CPU mode")
    x = make_data(a.chains, a.iters, a.cols, 0)
    dx = torch.as_tensor(x, device="cuda:0")
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        got = chain_diagnostics(dx, burn=a.burn)
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        got = chain_diagnostics(dx, burn=a.burn)
        times.append(time.perf_counter() - t0)
    n = (a.iters - a.burn) // 2
    out = {
        "shape": [a.chains, a.iters, a.cols],
        "bytes": int(x.nbytes),
        "device_ms_best": 1e3 * min(times),
        "device_ms_median": 1e3 * float(np.median(times)),
        "lag_blocks": lag_blocks(got["max_lag"], n),
        "max_lag": int(got["max_lag"].max()),
        "ess_min": float(np.nanmin(got["ess"])),
        "r_hat_max": float(np.nanmax(got["r_hat"])),
    }
    if not a.no_reference:
        t0 = time.perf_counter()
        ref = R.diagnostics(x, burn=a.burn)
        out["numpy_reference_s"] = time.perf_counter() - t0
        out["max_rel_err"] = {k: float(np.nanmax(np.abs(got[k] / ref[k] - 1)))
                              for k in ("r_hat", "ess", "sd")}
        out["max_lag_equal"] = bool(np.array_equal(got["max_lag"], ref["max_lag"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
