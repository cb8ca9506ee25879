"""Time ``power_scale_sensitivity`` under the Student-t likelihood next to the Gaussian call on the
same device arrays in the same process (the pattern of scripts/sens_bench.py).

Two sizes: the 629 x 3 golden problem with two chains of 5 000 draws, and the headline one, (64
chains, 50 000 draws, 33 columns) f64 of a 10 000 x 32 problem (draws scattered about the
least-squares point, made on the device).  Three calls alternate, --reps rounds after --warmup
rounds: the Gaussian call, ``nu=4`` and ``nu_draws=`` (a nu per draw cycling through seven values,
with their prior).  Per call: the library's own HIP events on its stream (bmc_sens_last_timing: the
log densities -- the Student-t pass counts there --, the sorts, the Pareto smoothing, the
distances) and the host clock around it (every call ends in a stream synchronise; the host clock of
the nu_draws call also holds the tabulation of the draws on the host).  Reports the medians, each
Student-t call's ratio to the Gaussian one and the share of the log-density stage.  Prints one JSON
line per size.
Usage: python scripts/sens_t_bench.py [--chains 64 --iters 50000 --points 10000 --k 32 --reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NU_GRID = np.array([1.5, 2.5, 4.0, 7.0, 12.0, 25.0, 50.0])
NU_WEIGHT = np.array([1.0, 3.0, 5.0, 4.0, 3.0, 2.0, 1.0])


def measure(name, A, y, samples, prior, Vt, warmup, reps):
    from pybmc_amd import _lib, power_scale_sensitivity
    ctx = _lib.default_context(0)
    lead = tuple(samples.shape[:-1])
    draws = NU_GRID[np.arange(int(np.prod(lead))) % len(NU_GRID)].reshape(lead)
    calls = {"gaussian": {}, "nu4": {"nu": 4.0},
             "nu_per_draw": {"nu_draws": draws, "nu_grid": NU_GRID, "nu_prior": NU_WEIGHT}}
    host = {c: [] for c in calls}
    parts = {c: [] for c in calls}
    for r in range(warmup + reps):
        for c, kw in calls.items():
            t0 = time.perf_counter()
            power_scale_sensitivity(A, y, samples, prior, Vt, **kw)
            t1 = time.perf_counter()
            if r >= warmup:
                host[c].append(1e3 * (t1 - t0))
                parts[c].append(ctx.sens_last_timing())
    med = lambda v: float(np.median(v))
    out = {"case": name, "samples_shape": list(samples.shape), "problem_shape": list(A.shape),
           "n_models": 0 if Vt is None else int(Vt.shape[1]), "reps": reps}
    for c in calls:
        split = {k: med([p[k] for p in parts[c]]) for k in parts[c][0]}
        device = [sum(p.values()) for p in parts[c]]
        out[c] = {"device_ms_median": med(device), "device_ms_min": min(device), "device_ms_max": max(device),
                  "host_ms_median": med(host[c]), "split_ms_median": split,
                  "logdens_share": split["logdens_ms"] / sum(split.values())}
    for c in ("nu4", "nu_per_draw"):
        out[c]["device_ratio_to_gaussian"] = out[c]["device_ms_median"] / out["gaussian"]["device_ms_median"]
        out[c]["logdens_ratio_to_gaussian"] = (out[c]["split_ms_median"]["logdens_ms"] /
                                               out["gaussian"]["split_ms_median"]["logdens_ms"])
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=64)
    ap.add_argument("--iters", type=int, default=50000)
    ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()

    import torch
    from pybmc_amd import gibbs_sampler

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: sens_t_bench measures the device and has no CPU mode")
    with np.load(os.path.join(ROOT, "tests", "golden", "gibbs_ortho629x3.npz"), allow_pickle=False) as g:
        X, yg, Vt = g["X"], g["y"], g["Vt"]
        prior = [g["b0"], g["C0"], float(g["nu0"]), float(g["s20"])]
    chains = gibbs_sampler(yg, X, 5000, prior, n_chains=2, seeds=[1, 2])
    dchains = torch.as_tensor(chains, device="cuda:0")
    torch.cuda.synchronize()
    measure("golden629x3", X, yg, dchains, prior, Vt, a.warmup, a.reps)
    del dchains

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
    measure("headline", A, y, samples, [np.zeros(k), np.eye(k) * 4.0, 1.0, 0.02], None, a.warmup, a.reps)


if __name__ == "__main__":
    main()
