#!/usr/bin/env python3
"""Record the goldens of tests/test_row_sum_classes_gpu.py: the chains of the library AS BUILT on
the cases of tests/row_sum_cases.py.

    python scripts/record_row_sum_golden.py [--lib path/to/libpybmc_amd.so] [--out DIR]

Run it ONCE, on an MI355X, at the commit whose bits are to be kept (the parent of a change to the
leader's row sum or to the residual pass); the test then holds every later build to those bits
with np.array_equal.  A case is recorded only if its chain is finite and ran in the geometry it
asks for, and the pair only if its chain 0 equals the chain run alone.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import row_sum_cases as rc  # noqa: E402
from pybmc_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=_lib.LIB_PATH)
    ap.add_argument("--out", default=rc.GOLDEN_DIR)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    _lib._share_hip_runtime_with_torch()
    ctx = _lib.Context(0, lib=_lib.bind(os.path.abspath(args.lib)))

    def save(name, a):
        assert np.isfinite(a).all(), name
        np.save(os.path.join(args.out, name + ".npy"), a)

    for name in rc.CASES:
        out, st = rc.run_case(ctx, name)
        save(name, out)
        print(f"{name}: G={st['groups_per_chain']} W={st['waves_per_group']} local={st['xcd_local_chains']} "
              f"-> {out.shape}  {ctx.last_kernels()}", flush=True)
    pair, alone, st = rc.run_pair(ctx)
    assert np.array_equal(pair[0], alone), rc.PAIR
    assert not np.array_equal(pair[0], pair[1]), rc.PAIR
    save(rc.PAIR, pair)
    print(f"{rc.PAIR}: G={st['groups_per_chain']} W={st['waves_per_group']} -> {pair.shape}", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
