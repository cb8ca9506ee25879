"""Time the posterior predictive with Student-t noise made on the device (``bmc_predict_t``,
``bmc_predict_tv``; predict_gemm_kernel<PG_T / PG_TV>, kernels_predict.hip) next to the Gaussian call
and next to the host-noise path.

  (a) kernel   ``gemm_ms`` and ``orderstat_ms`` of ``bmc_predict_timing`` for the Gaussian call, nu = 4,
               a nu per draw (64 distinct values between 1.5 and 50), nu = 1.5 and nu = 50 (how heavy
               tails load the order statistics), alternating in one process: medians of --reps after
               --warmup of each.  Shapes: 629 points x 4 models, k = 3, and 50 000 points x 257 models,
               k = 32, both with 10 000 draws.
  (b) call     the host clock around ``rndm_m_random_calculator(noise_df=4.0)`` with
               ``noise_source="host"`` and ``"device"``, alternating, medians of --call-reps after one
               warm-up of each, and the Gaussian call (``noise_df=None``) beside them.  Shapes: 629 x 4
               and 5 000 x 257: the host path is linear in the points, and a tenth of the large shape
               keeps the run short.

One JSON line per (part, shape).  Without --step every (part, shape) runs as a process of its own under
``timeout``, one after the other, and the run stops at the first that fails.
Usage: python scripts/predict_t_bench.py [--reps 5] [--warmup 2] [--call-reps 3]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_DRAWS = 10000
KERNEL_SHAPES = {"reference_size": (629, 4, 3), "c5": (50000, 257, 32)}
CALL_SHAPES = {"reference_size": (629, 4, 3), "c5_tenth": (5000, 257, 32)}
NU = 4.0
NU_VALUES = 64
# (part, shape, seconds): sized to the step
STEPS = [("kernel", "reference_size", 120), ("kernel", "c5", 300), ("call", "reference_size", 120),
         ("call", "c5_tenth", 420)]


def make_case(M, Km, k, S, seed=0):
    rng = np.random.default_rng(seed)
    preds = rng.standard_normal((M, Km)) + 3
    theta = np.column_stack([rng.standard_normal((S, k)) * 0.1, rng.uniform(0.5, 1.5, S)])
    Vt = rng.standard_normal((k, Km))
    return preds, theta, Vt


def kernel_step(name, a):
    from pybmc_amd import _lib
    M, Km, k = KERNEL_SHAPES[name]
    ctx = _lib.default_context(0)
    preds, theta, Vt = make_case(M, Km, k, N_DRAWS)
    nus = np.random.default_rng(1).choice(np.geomspace(1.5, 50.0, NU_VALUES), N_DRAWS)
    noise = {"gauss": {}, "t": {"nu": NU}, "tv": {"nu_draws": nus}, "t_nu1.5": {"nu": 1.5},
             "t_nu50": {"nu": 50.0}}

    def run(key):
        ctx.predict(preds, theta, Vt, seed=12345, want_draws=False, **noise[key])
        return ctx.predict_timing()

    for _ in range(a.warmup):
        for key in noise:
            run(key)
    gemm = {key: [] for key in noise}
    order = {key: [] for key in noise}
    for _ in range(a.reps):
        for key in noise:
            tm = run(key)
            gemm[key].append(tm["gemm_ms"])
            order[key].append(tm["select_ms"])
    g = {key: float(np.median(v)) for key, v in gemm.items()}
    o = {key: float(np.median(v)) for key, v in order.items()}
    print(json.dumps({"part": "kernel", "shape": name, "n_points": M, "n_models": Km, "k": k,
                      "n_draws": N_DRAWS, "nu": NU, "nu_values": NU_VALUES, "reps": a.reps,
                      "gemm_ms_median": g, "orderstat_ms_median": o, "gemm_ms_all": gemm,
                      "orderstat_ms_all": order, "t_over_gauss": g["t"] / g["gauss"],
                      "tv_over_gauss": g["tv"] / g["gauss"],
                      "orderstat_nu1.5_over_nu50": o["t_nu1.5"] / o["t_nu50"]}), flush=True)


def call_step(name, a):
    from pybmc_amd.sampling_utils import rndm_m_random_calculator
    M, Km, k = CALL_SHAPES[name]
    preds, samples, Vt = make_case(M, Km, k, N_DRAWS + 2000)
    calls = {"host": {"noise_df": NU, "noise_source": "host"},
             "device": {"noise_df": NU, "noise_source": "device"}, "gauss": {}}

    def timed(kw):
        t0 = time.perf_counter()
        rndm_m_random_calculator(preds, samples, Vt, seed=12345, **kw)
        return (time.perf_counter() - t0) * 1e3

    for kw in calls.values():
        timed(kw)
    ms = {key: [] for key in calls}
    for _ in range(a.call_reps):
        for key, kw in calls.items():
            ms[key].append(timed(kw))
    med = {key: float(np.median(v)) for key, v in ms.items()}
    note = ("a tenth of the 50 000-point shape: the host path is linear in the points"
            if name == "c5_tenth" else "")
    print(json.dumps({"part": "call", "shape": name, "n_points": M, "n_models": Km, "k": k,
                      "n_draws": N_DRAWS, "nu": NU, "reps": a.call_reps, "call_ms_median": med,
                      "call_ms_all": ms, "host_over_device": med["host"] / med["device"],
                      "device_over_gauss": med["device"] / med["gauss"], "note": note}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--call-reps", type=int, default=3)
    ap.add_argument("--step", default=None, help="part:shape, run in this process")
    a = ap.parse_args()
    if a.step is not None:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("no GPU: predict_t_bench measures the device and has no CPU mode")
        part, name = a.step.split(":")
        (kernel_step if part == "kernel" else call_step)(name, a)
        return
    for part, name, seconds in STEPS:
        rc = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__),
                             "--step", f"{part}:{name}", "--warmup", str(a.warmup), "--reps", str(a.reps),
                             "--call-reps", str(a.call_reps)]).returncode
        if rc != 0:
            raise SystemExit(f"step {part}:{name} ended with status {rc}; nothing further is started")


if __name__ == "__main__":
    main()
