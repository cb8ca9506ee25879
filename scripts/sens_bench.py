"""Time ``power_scale_sensitivity`` on device arrays next to ``rank_diagnostics`` on the same sample
array in the same process.

Two sizes: the headline one, (64 chains, 50 000 draws, 33 columns) f64 = 845 MB of draws of a
10 000 x 32 problem (draws scattered about the least-squares point, on the device), and the
629 x 3 golden problem with two Gibbs chains of 5 000 draws.  The two calls alternate, --reps
rounds after --warmup rounds.  Per call: the host clock around it (both end in a stream
synchronise), and for the sensitivity the library's own HIP events on its stream
(bmc_sens_last_timing): the log densities, the sorts (gathers included), the Pareto smoothing, the
distances.  Reports best and median of each, the per-pass shares and the ratio of the medians.
Prints one JSON line per size.
Usage: python scripts/sens_bench.py [--chains 64 --iters 50000 --points 10000 --k 32 --reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(name, A, y, samples, prior, Vt, warmup, reps, cols_per_batch):
    from pybmc_amd import _lib, power_scale_sensitivity, rank_diagnostics
    ctx = _lib.default_context(0)
    sens_t, rank_t, parts = [], [], []
    res = None
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        rank_diagnostics(samples)
        t1 = time.perf_counter()
        res = power_scale_sensitivity(A, y, samples, prior, Vt, cols_per_batch=cols_per_batch)
        t2 = time.perf_counter()
        if r >= warmup:
            rank_t.append(1e3 * (t1 - t0))
            sens_t.append(1e3 * (t2 - t1))
            parts.append(ctx.sens_last_timing())
    med = lambda v: float(np.median(v))
    split = {k: med([p[k] for p in parts]) for k in parts[0]}
    total = sum(split.values())
    out = {
        "case": name, "samples_shape": list(samples.shape), "problem_shape": list(A.shape),
        "n_models": 0 if Vt is None else int(Vt.shape[1]), "cols_per_batch": cols_per_batch,
        "sens_ms_best": min(sens_t), "sens_ms_median": med(sens_t),
        "rank_ms_best": min(rank_t), "rank_ms_median": med(rank_t),
        "ratio_median": med(sens_t) / med(rank_t),
        "split_ms_median": split, "device_ms_median": total,
        "share": {k: v / total for k, v in split.items()},
        "psens_prior_max": float(np.nanmax(res["psens"]["prior"])),
        "psens_likelihood_max": float(np.nanmax(res["psens"]["likelihood"])),
        "pareto_k": {c: [float(v) for v in res["pareto_k"][c]] for c in res["components"]},
    }
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=64)
    ap.add_argument("--iters", type=int, default=50000)
    ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cols-per-batch", type=int, default=0)
    a = ap.parse_args()

    import torch
    from pybmc_amd import gibbs_sampler

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: sens_bench measures the device and has no CPU mode")
    rng = np.random.default_rng(0)
    N, k = a.points, a.k
    A = rng.standard_normal((N, k)) / np.sqrt(N)
    btrue = rng.standard_normal(k)
    y = A @ btrue + 0.3 * rng.standard_normal(N)
    bhat = np.linalg.lstsq(A, y, rcond=None)[0]
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    z = torch.randn((a.chains, a.iters, k + 1), dtype=torch.float64, device="cuda:0", generator=gen)
    samples = torch.empty_like(z)
    samples[..., :k] = torch.as_tensor(bhat, device="cuda:0") + 0.3 * z[..., :k]   # sd of a coefficient
    samples[..., k] = 0.3 * torch.exp(z[..., k] / np.sqrt(2.0 * N))
    del z
    torch.cuda.synchronize()
    prior = [np.zeros(k), np.eye(k) * 4.0, 1.0, 0.02]
    measure("headline", A, y, samples, prior, None, a.warmup, a.reps, a.cols_per_batch)
    del samples
    torch.cuda.empty_cache()

    with np.load(os.path.join(ROOT, "tests", "golden", "gibbs_ortho629x3.npz"), allow_pickle=False) as g:
        X, yg, Vt = g["X"], g["y"], g["Vt"]
        prior = [g["b0"], g["C0"], float(g["nu0"]), float(g["s20"])]
    chains = gibbs_sampler(yg, X, 5000, prior, n_chains=2, seeds=[1, 2])
    dchains = torch.as_tensor(chains, device="cuda:0")
    torch.cuda.synchronize()
    measure("golden629x3", X, yg, dchains, prior, Vt, a.warmup, a.reps, a.cols_per_batch)


if __name__ == "__main__":
    main()
