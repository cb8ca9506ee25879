#!/usr/bin/env python3
"""Record the goldens of tests/test_hit_path_gpu.py: the chains of the library AS BUILT on the
cases of tests/hit_path_cases.py.

    python scripts/record_hit_path_golden.py [--lib path/to/libpybmc_amd.so] [--out DIR]

Run it ONCE, on an MI355X, at the commit whose bits are to be kept (the parent of a change to the
leader's gather or to its sigma2 step); the test then holds every later build to those bits with
np.array_equal.  A case is recorded only if its chain is finite and ran in the geometry it asks
for; the trio only if its chain 0 equals the chain run alone; the floor case only if the device
chain sits on the floor in some rows and not in others.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hit_path_cases as hc  # noqa: E402
from pybmc_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=_lib.LIB_PATH)
    ap.add_argument("--out", default=hc.GOLDEN_DIR)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    _lib._share_hip_runtime_with_torch()
    ctx = _lib.Context(0, lib=_lib.bind(os.path.abspath(args.lib)))

    def save(name, a):
        assert np.isfinite(a).all(), name
        np.save(os.path.join(args.out, name + ".npy"), a)

    for name in hc.CASES:
        out, st = hc.run_case(ctx, name)
        save(name, out)
        print(f"{name}: G={st['groups_per_chain']} W={st['waves_per_group']} local={st['xcd_local_chains']} "
              f"-> {out.shape}  {ctx.last_kernels()}", flush=True)
    chains, _ = hc.run_stale(ctx)
    assert not np.array_equal(chains[0], chains[1]), hc.STALE
    for name, a in zip(hc.STALE, chains):
        save(name, a)
        print(f"{name}: -> {a.shape}", flush=True)
    trio, alone, st = hc.run_trio(ctx)
    assert np.array_equal(trio[0], alone), hc.TRIO
    assert not np.array_equal(trio[0], trio[1]), hc.TRIO
    save(hc.TRIO, trio)
    print(f"{hc.TRIO}: G={st['groups_per_chain']} W={st['waves_per_group']} -> {trio.shape}", flush=True)
    out, st = hc.run_floor(ctx)
    on_floor = np.isclose(out[:, -1], np.sqrt(hc.SIGMA2_FLOOR), rtol=1e-12, atol=0.0)
    assert on_floor.any() and not on_floor.all(), on_floor
    save(hc.FLOOR, out)
    print(f"{hc.FLOOR}: G={st['groups_per_chain']} W={st['waves_per_group']} -> {out.shape}, "
          f"{int(on_floor.sum())} of {len(on_floor)} rows on the floor", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
