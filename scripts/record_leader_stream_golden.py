#!/usr/bin/env python3
"""Record the goldens of tests/test_leader_stream_gpu.py: the chains of the library AS BUILT on the
cases of tests/leader_stream_cases.py.

    python scripts/record_leader_stream_golden.py [--lib path/to/libpybmc_amd.so] [--out DIR]

Run it ONCE, on an MI355X, at the commit whose bits are to be kept (the parent of a change to the
leader wave's loop); the test then holds every later build to those bits with np.array_equal.  A
case is recorded only if its chains are finite, a shorter run is the prefix of the longer one of
its shape, and a chain run beside others equals the chain run alone.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import leader_stream_cases as lc  # noqa: E402
from pybmc_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=_lib.LIB_PATH)
    ap.add_argument("--out", default=lc.GOLDEN_DIR)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    _lib._share_hip_runtime_with_torch()
    ctx = _lib.Context(0, lib=_lib.bind(os.path.abspath(args.lib)))

    def save(name, a):
        assert np.isfinite(a).all(), name
        np.save(os.path.join(args.out, name + ".npy"), a)

    longest = {}
    for name in lc.GIBBS_CASES:
        out, st = lc.run_gibbs_case(ctx, name)
        save(name, out)
        key = name.rsplit("_t", 1)[0]
        if out.shape[0] == lc.T_MAX:
            longest[key] = out
        print(f"{name}: G={st['groups_per_chain']} W={st['waves_per_group']} local={st['xcd_local_chains']} "
              f"-> {out.shape}  {ctx.last_kernels()}", flush=True)
    for name in lc.GIBBS_CASES:      # (a run of T iterations is the first T rows of the run of 65)
        key = name.rsplit("_t", 1)[0]
        if key in longest:
            out = np.load(os.path.join(args.out, name + ".npy"))
            assert np.array_equal(out, longest[key][:out.shape[0]]), name
    for name, replay in ((lc.PAIR_REPLAY, True), (lc.PAIR_DEVICE, False)):
        pair, alone, st = lc.run_pair(ctx, replay)
        assert np.array_equal(pair[0], alone), name
        assert not np.array_equal(pair[0], pair[1]), name
        save(name, pair)
        print(f"{name}: G={st['groups_per_chain']} W={st['waves_per_group']} -> {pair.shape}", flush=True)
    out, st = lc.run_pack16(ctx)
    ctx.set_tuning(**lc.PACK_TUNING)
    for c in range(16):
        alone, st1 = lc.run_replay(ctx, 640, 16, 3, (c,))
        assert st1["groups_per_chain"] == st["groups_per_chain"], (st, st1)
        assert np.array_equal(out[c], alone[0]), (lc.PACK16, c)
    ctx.set_tuning()
    save(lc.PACK16, out)
    print(f"{lc.PACK16}: G={st['groups_per_chain']} W={st['waves_per_group']} cpp={st['chains_per_pass']} "
          f"-> {out.shape}", flush=True)
    out, acc, used, st = lc.run_simplex_case(ctx)
    save(lc.SIMPLEX_CASE, out)
    print(f"{lc.SIMPLEX_CASE}: G={st['groups_per_chain']} W={st['waves_per_group']} accepted {acc} "
          f"uniforms {used} -> {out.shape}", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
