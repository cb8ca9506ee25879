"""Every call of the granule gather keeps the bits it had before the trailing poll was retired
behind the group sum (-m gpu): first level with workgroup-scope and agent-scope stores, team totals
and second level, 16 chains per launch, bundles of 8, and the simplex sampler.  The goldens under
tests/golden/gather_tail/ were recorded by scripts/record_gather_tail_golden.py at the commit before
that change; a chain must equal its golden with np.array_equal -- where a poll is waited for may
move, what is summed and in which order may not.  The many-chain cases are also compared slot by
slot with the chain run alone in the same geometry."""
import os

import numpy as np
import pytest

import gather_tail_cases as gc
from gpu_common import gpu_ctx

pytestmark = pytest.mark.gpu


def golden(name):
    path = gc.golden_path(name)
    if not os.path.exists(path):
        pytest.skip(f"golden {os.path.basename(path)} not recorded")
    return np.load(path, allow_pickle=False)


@pytest.mark.parametrize("name", list(gc.GIBBS_CASES))
def test_gibbs_chain_is_the_parent_commits_bits(name):
    want = golden(name)
    out, alone, st = gc.run_gibbs_case(gpu_ctx(), name)
    print(f"{name}: {st}")
    assert out.shape[1:] == want.shape
    if alone is not None:
        assert np.array_equal(alone[0], want), (name, "alone", st)
    for c in range(out.shape[0]):
        assert np.array_equal(out[c], want), (name, c, st)


def test_simplex_chain_is_the_parent_commits_bits():
    want = golden(gc.SIMPLEX_CASE)
    out, acc, used, st = gc.run_simplex_case(gpu_ctx())
    print(f"{gc.SIMPLEX_CASE}: accepted {acc}, uniforms {used}, {st}")
    assert np.array_equal(out, want), st
