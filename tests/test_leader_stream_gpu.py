"""The leader wave's loop keeps the bits it had before its loop control was trimmed (-m gpu): one
remaining-iterations counter, variate pointers advanced by an add, a prefetch that is no longer
skipped in the last iteration (it reads the row behind the chain's last one: the next chain's
first row, or the padding row behind the last chain), a 32-bit abort test and a gather that carries
no flag.  The goldens under tests/golden/leader_stream/ were recorded by
scripts/record_leader_stream_golden.py at the commit before that change; a chain must equal its
golden with np.array_equal -- instructions and their schedule may move, what is computed may not."""
import os

import numpy as np
import pytest

import leader_stream_cases as lc
from gpu_common import gpu_ctx

pytestmark = pytest.mark.gpu


def golden(name):
    path = lc.golden_path(name)
    assert os.path.exists(path), f"golden {os.path.basename(path)} not recorded"
    return np.load(path, allow_pickle=False)


@pytest.mark.parametrize("name", list(lc.GIBBS_CASES))
def test_gibbs_chain_is_the_parent_commits_bits(name):
    """k = 16 over 2 and 32 groups at T = 1, 2, 3 and 65 (the unused last prefetch, both slot
    parities), k = 5 (no DPP block) and k = 40 (lanes 40..63 draw 0), the headline kernel in the
    planner's geometry, and agent scope forced."""
    want = golden(name)
    out, st = lc.run_gibbs_case(gpu_ctx(), name)
    print(f"{name}: {st}")
    assert out.shape == want.shape
    assert np.array_equal(out, want), (name, st)


def test_headline_case_runs_the_headline_kernel():
    ctx = gpu_ctx()
    lc.run_gibbs_case(ctx, "headline_t65")
    names = ctx.last_kernels()
    print(names)
    assert len(names) == 1 and "gibbs_loop_kernel<double, 1, 0, 32, 1, false, false, true>" in names[0], names


@pytest.mark.parametrize("name,replay", [(lc.PAIR_REPLAY, True), (lc.PAIR_DEVICE, False)])
def test_chain_beside_another_stream_equals_the_chain_alone(name, replay):
    """Two chains with streams of their own at T = 2: chain 0's unused prefetch lands in chain 1's
    first row, chain 1's in the padding row -- with uploaded streams and with the device's."""
    want = golden(name)
    pair, alone, st = lc.run_pair(gpu_ctx(), replay)
    print(f"{name}: {st}")
    assert np.array_equal(pair[0], alone), (name, st)
    assert np.array_equal(pair, want), (name, st)


def test_short_run_after_a_long_one_on_one_context():
    """T = 65 and then T = 2 on the same context: nothing of the first run -- its padding row, its
    pointers -- reaches the second."""
    ctx = gpu_ctx()
    for name in ("k16_g2_t65", "k16_g2_t2", "k16_g32_t65", "k16_g32_t1"):
        out, st = lc.run_gibbs_case(ctx, name)
        assert np.array_equal(out, golden(name)), (name, st)


def test_sixteen_chains_packed_are_the_parent_commits_bits():
    want = golden(lc.PACK16)
    ctx = gpu_ctx()
    out, st = lc.run_pack16(ctx)
    print(f"{lc.PACK16}: {st}")
    assert np.array_equal(out, want), st
    # the last chain of the launch alone: its unused prefetch reads the padding row either way
    ctx.set_tuning(**lc.PACK_TUNING)
    try:
        alone, _ = lc.run_replay(ctx, 640, 16, 3, (15,))
    finally:
        ctx.set_tuning()
    assert np.array_equal(alone[0], want[15])


def test_simplex_chain_is_the_parent_commits_bits():
    want = golden(lc.SIMPLEX_CASE)
    out, acc, used, st = lc.run_simplex_case(gpu_ctx())
    print(f"{lc.SIMPLEX_CASE}: accepted {acc}, uniforms {used}, {st}")
    assert np.array_equal(out, want), st
