#!/usr/bin/env python3
"""Record the goldens of tests/test_scorer_golden_gpu.py: what the scorers of the library AS BUILT
(psis_loo and its Student-t and predictive forms, pointwise_loglik, ppc, power_sensitivity, the
rank-normalised diagnostics) return on the cases of tests/scorer_golden_cases.py.

    python scripts/record_scorer_golden.py [--lib path/to/libpybmc_amd.so] [--out DIR]

Run it ONCE, on an MI355X, at the commit whose bits are to be kept (the parent of a change to the
Pareto tail fit, the staging kernels or the key gather); the test then holds every later build to
those bits.  --lib names a saved build of that commit.  Every call is made twice and recorded
only if the two agree bit for bit.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scorer_golden_cases as sc  # noqa: E402
from pybmc_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=_lib.LIB_PATH)
    ap.add_argument("--out", default=sc.GOLDEN_DIR)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    _lib._share_hip_runtime_with_torch()
    ctx = _lib.Context(0, lib=_lib.bind(os.path.abspath(args.lib)))
    for family, run in sc.FAMILIES.items():
        flat, again = sc.flatten(run(ctx)), sc.flatten(run(ctx))
        assert list(flat) == list(again), family
        for name, v in flat.items():
            assert v.shape == again[name].shape and np.array_equal(v, again[name]), (family, name)
        for i, arrays in enumerate(sc.split_files(flat)):
            path = os.path.join(args.out, f"{family}.{i}.npz")
            np.savez(path, **arrays)
            size = os.path.getsize(path)
            assert size <= sc.FILE_BYTES, (path, size)
            print(f"{family}.{i}: {len(arrays)} arrays -> {size} bytes", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
