"""Time the pointwise log-likelihood / WAIC kernels (``pybmc_amd.scoring``) on device arrays.

Shapes: C1 (377 x 3, 50 000 draws), C2 (10 000 x 32, 50 000 draws) and C2 with 8 pooled chains
(400 000 draws).  Device time: HIP events on the library's stream around one call of the device
entry point (pad, per-draw constants, tile kernel, merge and the copy of the three result vectors),
best and median of --reps calls after --warmup calls.  Reported against
  * the chunked numpy reference of the tests on the same host (first two shapes), and
  * the MFMA floor: ceil(n/16) ceil(S/16) ceil(k/4) v_mfma_f64_16x16x4_f64 of 64 cycles each over
    1024 SIMDs at --clock-ghz (an assumption: the clock is not read during the run),
as achieved f64 TF (2 n S k useful flops) and the MFMA-busy share floor / time.
Then the use case: a sweep of ``components_kept`` on a synthetic frame with three true components,
``elpd_waic`` on the training rows and held-out ``elpd`` on a validation split per value.
One JSON line per measurement.  Usage: python scripts/score_bench.py [--reps 7] [--no-reference]
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

SHAPES = [("c1", 377, 3, 50000), ("c2", 10000, 32, 50000), ("c2_8chains", 10000, 32, 400000)]


def make_case(n, k, S, seed):
    rng = np.random.default_rng(seed)
    A = np.linalg.qr(rng.standard_normal((n, k)))[0]
    b = rng.standard_normal(k)
    y = A @ b + 0.1 * rng.standard_normal(n)
    sig = 0.1 * (1 + rng.standard_normal(S) / np.sqrt(2 * n))
    return A, y, np.column_stack([A.T @ y + sig[:, None] * rng.standard_normal((S, k)), sig])


def mfma_floor_ms(n, k, S, clock_ghz):
    tiles = -(-n // 16) * -(-S // 16) * -(-k // 4)       # 16 x 16 x 4 MFMAs
    return tiles * 64 / 1024 / (clock_ghz * 1e9) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--no-sweep", action="store_true")
    a = ap.parse_args()

    import torch
    import score_reference as R
    from pybmc_amd import _lib

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: score_bench measures the device and has no CPU mode")
    dev = torch.device("cuda", 0)
    ctx = _lib.default_context(0)
    stream = torch.cuda.Stream(dev)
    ctx.set_stream(stream.cuda_stream)
    for name, n, k, S in SHAPES:
        A, y, th = make_case(n, k, S, 0)
        dA, dy, dth = (torch.as_tensor(v, device=dev) for v in (A, y, th))
        torch.cuda.synchronize()

        def call():
            return ctx.pointwise_loglik_device(dA.data_ptr(), n, k, k, _lib.BMC_ROW_MAJOR,
                                               dy.data_ptr(), dth.data_ptr(), S, k + 1)
        for _ in range(a.warmup):
            got = call()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            got = call()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        best = min(ms)
        floor = mfma_floor_ms(n, k, S, a.clock_ghz)
        out = {"shape": name, "n_points": n, "k": k, "n_draws": S, "device_ms_best": best,
               "device_ms_median": float(np.median(ms)), "f64_tflops": 2.0 * n * S * k / best / 1e9,
               "mfma_floor_ms": floor, "mfma_busy_share": floor / best,
               "elements_per_ns": n * S / best / 1e6, "clock_ghz_assumed": a.clock_ghz}
        if not a.no_reference and name != "c2_8chains":
            t0 = time.perf_counter()
            ref = R.pointwise(A, y, th)
            out["numpy_reference_s"] = time.perf_counter() - t0
            out["max_err"] = {
                "lppd": float(np.max(np.abs(got["lppd"] - ref["lppd"]) / np.maximum(1, np.abs(ref["lppd"])))),
                "p_waic": float(np.max(np.abs(got["p_waic"] / ref["p_waic"] - 1))),
                "mean_ll": float(np.max(np.abs(got["mean_ll"] / ref["mean_ll"] - 1)))}
        print(json.dumps(out), flush=True)
        del dA, dy, dth
    ctx.set_stream(None)

    if a.no_sweep:
        return
    from pybmc_amd import BayesianModelCombination
    train, models = R.three_component_frame(400, seed=1)
    val, _ = R.three_component_frame(200, seed=2)
    import contextlib
    import io
    for kept in range(1, len(models)):
        b = BayesianModelCombination(models, {"p": train}, truth_column_name="truth")
        b.orthogonalize("p", train, components_kept=kept, method="svd")
        with contextlib.redirect_stdout(io.StringIO()):
            b.train({"iterations": 20000, "burn": 2000, "n_chains": 4, "seeds": [1, 2, 3, 4]})
        w, h = b.waic(), b.log_predictive_density(val)
        print(json.dumps({"components_kept": kept, "elpd_waic": w["elpd_waic"], "se": w["se"],
                          "p_waic": w["p_waic"], "n_high_p": w["n_high_p"],
                          "held_out_elpd": h["elpd"], "held_out_se": h["se"]}), flush=True)


if __name__ == "__main__":
    main()
