"""The leader's gather decides on the tags of all 64 lanes and polls through one asm statement; the
chains keep the bits they had (-m gpu).  The goldens under tests/golden/hit_path/ were recorded by
scripts/record_hit_path_golden.py at the commit before the change, and a chain must equal its
golden with np.array_equal.  The expiry of the bounded spin is not provoked here (nor anywhere):
its way through the code is described in DESIGN.md 4.1."""
import os

import numpy as np
import pytest

import hit_path_cases as hc
from gpu_common import gpu_ctx

pytestmark = pytest.mark.gpu


def golden(name):
    path = hc.golden_path(name)
    assert os.path.exists(path), f"golden {os.path.basename(path)} not recorded"
    return np.load(path, allow_pickle=False)


@pytest.mark.parametrize("name", list(hc.CASES))
def test_chain_is_the_parent_commits_bits(name):
    """2, 3, 5, 31 and 32 groups in the scope the placement check finds and at agent scope (the
    lanes past the last granule decide with the others), the headline instantiation at two waves
    per group, and chains of one, two and three iterations; each case asserts the geometry it ran
    in (hit_path_cases.run_case)."""
    want = golden(name)
    out, st = hc.run_case(gpu_ctx(), name)
    print(f"{name}: {st}")
    assert out.shape == want.shape
    assert np.array_equal(out, want), (name, st)


def test_headline_case_runs_the_headline_kernel():
    ctx = gpu_ctx()
    hc.run_case(ctx, hc.HEADLINE)
    names = ctx.last_kernels()
    print(names)
    assert len(names) == 1 and hc.HEADLINE_KERNEL in names[0], names


def test_a_launch_takes_no_granule_of_the_launch_before_it():
    """Two launches back to back on one context: the granules of the first are still in the
    exchange area, with all their tags alike, when the second starts; its nonce keeps them out."""
    chains, stats = hc.run_stale(gpu_ctx())
    print(stats)
    for name, out in zip(hc.STALE, chains):
        assert np.array_equal(out, golden(name)), name


def test_chain_beside_two_others_equals_the_chain_alone():
    want = golden(hc.TRIO)
    trio, alone, st = hc.run_trio(gpu_ctx())
    print(f"{hc.TRIO}: {st}")
    assert np.array_equal(trio[0], alone), st
    assert np.array_equal(trio, want), st


def test_floor_of_the_sigma2_step_is_hit_and_keeps_its_bits():
    """First on the CPU: the oracle floors sigma2 in some iterations of these inputs and not in
    others.  Then the device chain: it sits on the floor in some rows and not in others, and equals
    the parent commit's bits."""
    hits = hc.floor_hits_on_the_cpu()
    print(f"oracle: {int(hits.sum())} of {len(hits)} iterations floored")
    assert hits.any() and not hits.all(), hits
    want = golden(hc.FLOOR)
    out, st = hc.run_floor(gpu_ctx())
    on_floor = np.isclose(out[:, -1], np.sqrt(hc.SIGMA2_FLOOR), rtol=1e-12, atol=0.0)
    print(f"{hc.FLOOR}: {st}; device: {int(on_floor.sum())} of {len(on_floor)} rows on the floor")
    assert on_floor.any() and not on_floor.all(), on_floor
    assert np.array_equal(out, want), st
