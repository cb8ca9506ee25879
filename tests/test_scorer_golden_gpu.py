"""The scorers keep their bits (-m gpu): psis_loo (Gaussian, Student-t, per-draw nu), psis_loo_predict,
pointwise_loglik, ppc, power_sensitivity and the rank-normalised diagnostics on the cases of
tests/scorer_golden_cases.py.  The goldens under tests/golden/scorers/ were recorded by
scripts/record_scorer_golden.py at the commit before the Pareto tail fit moved into bmc_psis.h and
the padding and gather kernels of the scorers became one each; every array must have the bit
pattern of its golden (np.array_equal on the uint64 view: a NaN is held as well) -- where a loop
is written may move, what it adds and in which order may not."""
import numpy as np
import pytest

import scorer_golden_cases as sc
from gpu_common import gpu_ctx

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("family", list(sc.FAMILIES))
def test_scorers_return_the_parent_commits_bits(family):
    want = {}
    for path in sc.golden_files(family):
        with np.load(path, allow_pickle=False) as z:
            want.update({name: z[name] for name in z.files})
    got = sc.flatten(sc.FAMILIES[family](gpu_ctx()))
    assert want and set(want) == set(got), family
    for name, v in got.items():
        differ = int((v != want[name]).sum()) if v.shape == want[name].shape else -1
        if differ:
            print(f"{family} {name}{v.shape}: {differ} elements differ from the golden")
    for name, v in got.items():
        assert np.array_equal(v, want[name]), (family, name)
