"""The leader's row sum at every wave count, and the residual pass, keep the bits they had
(-m gpu).  Every wave reads u first behind barrier B1, and the publishing lanes finish the wave
sum from their own row total; a form of the row sum that reads only the rows of waves that exist
must give these bits too.  None of that may change what is computed: the goldens under tests/golden/row_sum/
were recorded by scripts/record_row_sum_golden.py at the commit before the change, and a chain
must equal its golden with np.array_equal."""
import os

import numpy as np
import pytest

import row_sum_cases as rc
from gpu_common import gpu_ctx

pytestmark = pytest.mark.gpu


def golden(name):
    path = rc.golden_path(name)
    assert os.path.exists(path), f"golden {os.path.basename(path)} not recorded"
    return np.load(path, allow_pickle=False)


@pytest.mark.parametrize("name", list(rc.CASES))
def test_chain_is_the_parent_commits_bits(name):
    """One to eight waves per group with a ragged last panel, two to eight with an absent panel,
    two and four column blocks, and the headline geometry at agent scope; each case asserts the
    geometry it ran in (row_sum_cases.run_case)."""
    want = golden(name)
    out, st = rc.run_case(gpu_ctx(), name)
    print(f"{name}: {st}")
    assert out.shape == want.shape
    assert np.array_equal(out, want), (name, st)


def test_headline_geometry_at_agent_scope_runs_the_headline_kernel():
    ctx = gpu_ctx()
    rc.run_case(ctx, rc.HEADLINE_AGENT)
    names = ctx.last_kernels()
    print(names)
    assert len(names) == 1 and rc.HEADLINE_KERNEL in names[0], names


def test_chain_beside_another_stream_at_five_waves_equals_the_chain_alone():
    want = golden(rc.PAIR)
    pair, alone, st = rc.run_pair(gpu_ctx())
    print(f"{rc.PAIR}: {st}")
    assert np.array_equal(pair[0], alone), st
    assert np.array_equal(pair, want), st
