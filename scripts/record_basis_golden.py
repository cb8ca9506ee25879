#!/usr/bin/env python3
"""Record the goldens of tests/test_basis_golden_gpu.py: what set_prior, kfold_cv and
cv_component_path of the library AS BUILT return on the cases of tests/basis_golden_cases.py.

    python scripts/record_basis_golden.py [--lib path/to/libpybmc_amd.so] [--out DIR]

Run it ONCE, on an MI355X, at the commit whose bits are to be kept (the parent of a change to the
host algebra of the prior basis or to the cross-validation driver); the test then holds every
later build to those bits with np.array_equal.  --lib names a saved build of that commit; it
becomes the library of the device's shared context too, which kfold_cv, cv_component_path and
gibbs_sampler use.  Every call is made twice and recorded only if the two agree bit for bit.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import basis_golden_cases as bc  # noqa: E402
from pybmc_amd import _lib  # noqa: E402


def save(out_dir, files, again):
    for stem, arrays in files.items():
        for key, v in arrays.items():
            assert np.isfinite(v).all(), (stem, key)
            assert np.array_equal(v, again[stem][key]), (stem, key)
        path = os.path.join(out_dir, stem + ".npz")
        np.savez(path, **arrays)
        size = os.path.getsize(path)
        assert size <= 64 * 1024, (stem, size)
        print(f"{stem}: {', '.join(f'{k}{np.shape(v)}' for k, v in arrays.items())} -> {size} bytes",
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=_lib.LIB_PATH)
    ap.add_argument("--out", default=bc.GOLDEN_DIR)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    _lib._share_hip_runtime_with_torch()
    lib = _lib.bind(os.path.abspath(args.lib))
    ctx = _lib.Context(0, lib=lib)
    _lib._default_ctx[0] = _lib.Context(0, lib=lib)     # what the functional API runs on
    for name in bc.PRIOR_CASES:
        save(args.out, bc.run_prior_case(ctx, name), bc.run_prior_case(ctx, name))
    ctx.close()
    for name in bc.CV_CASES:
        save(args.out, bc.run_cv_case(name), bc.run_cv_case(name))


if __name__ == "__main__":
    main()
