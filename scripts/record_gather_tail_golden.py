#!/usr/bin/env python3
"""Record the goldens of tests/test_gather_tail_gpu.py: the chains of the library AS BUILT, in
replay mode, on the cases of tests/gather_tail_cases.py.

    python scripts/record_gather_tail_golden.py [--lib path/to/libpybmc_amd.so] [--out DIR]

Run it ONCE, on an MI355X, at the commit whose bits are to be kept (the parent of a change to the
granule gather); the test then holds every later build to those bits with np.array_equal.  A
many-chain case is recorded only if every slot is the same chain and equals the chain run alone.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gather_tail_cases as gc  # noqa: E402
from pybmc_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=_lib.LIB_PATH)
    ap.add_argument("--out", default=gc.GOLDEN_DIR)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    _lib._share_hip_runtime_with_torch()
    ctx = _lib.Context(0, lib=_lib.bind(os.path.abspath(args.lib)))
    for name in gc.GIBBS_CASES:
        out, alone, st = gc.run_gibbs_case(ctx, name)
        for c in range(out.shape[0]):
            assert np.array_equal(out[c], out[0]), (name, c)
        if alone is not None:
            assert np.array_equal(alone[0], out[0]), name
        assert np.isfinite(out[0]).all(), name
        np.save(os.path.join(args.out, name + ".npy"), out[0])
        print(f"{name}: {out.shape[0]} chain(s) G={st['groups_per_chain']} W={st['waves_per_group']} "
              f"cpp={st['chains_per_pass']} local={st['xcd_local_chains']} -> {out[0].shape}", flush=True)
    out, acc, used, st = gc.run_simplex_case(ctx)
    assert np.isfinite(out).all()
    np.save(os.path.join(args.out, gc.SIMPLEX_CASE + ".npy"), out)
    print(f"{gc.SIMPLEX_CASE}: G={st['groups_per_chain']} W={st['waves_per_group']} accepted {acc} "
          f"uniforms {used} -> {out.shape}", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
