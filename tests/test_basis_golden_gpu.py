"""What the prior-basis algebra decides keeps its bits (-m gpu): set_problem + set_prior (basis(),
conditional_moments(1.0), one default-rss and one rss="gram" chain), kfold_cv and
cv_component_path on the cases of tests/basis_golden_cases.py.  The goldens under
tests/golden/basis/ were recorded by scripts/record_basis_golden.py at the commit before the algebra
moved into bmc_basis.h and the cross-validation driver was cut into stages; every array must equal
its golden with np.array_equal -- where a loop is written may move, what it adds and in which
order may not.  One more test holds the order in which bmc_set_prior reports its errors."""
import numpy as np
import pytest

import basis_golden_cases as bc
from gpu_common import gpu_ctx

pytestmark = pytest.mark.gpu


def hold(files):
    for stem, arrays in files.items():
        with np.load(bc.golden_path(stem), allow_pickle=False) as want:
            assert set(want.files) == set(arrays), stem
            for key, got in arrays.items():
                got = np.asarray(got)
                differ = int((got != want[key]).sum()) if got.shape == want[key].shape else -1
                print(f"{stem} {key}{got.shape}: {differ} elements differ from the golden")
                assert np.array_equal(got, want[key]), (stem, key)


@pytest.mark.parametrize("name", list(bc.PRIOR_CASES))
def test_set_prior_is_the_parent_commits_bits(name):
    hold(bc.run_prior_case(gpu_ctx(), name))


@pytest.mark.parametrize("name", bc.CV_CASES)
def test_cross_validation_is_the_parent_commits_bits(name):
    hold(bc.run_cv_case(name))


def test_set_prior_reports_its_errors_in_order():
    """C0 singular, then X'X singular, then inv(C0) + 1e-6 I not positive definite"""
    rng = np.random.default_rng(3)
    X = rng.standard_normal((40, 3))
    X[:, 2] = 0.0                          # rank deficient: row 2 of X'X is exactly zero
    y = rng.standard_normal(40)
    ctx = gpu_ctx()
    ctx.set_problem(y, X)
    with pytest.raises(np.linalg.LinAlgError, match=r"Singular matrix \(b_mean_cov\)"):
        ctx.set_prior(np.zeros(3), np.ones((3, 3)), 1.0, 0.02)
    with pytest.raises(np.linalg.LinAlgError, match=r"Singular matrix \(X'X\)"):
        ctx.set_prior(np.zeros(3), -np.eye(3), 1.0, 0.02)
    ctx.set_problem(y, rng.standard_normal((40, 3)))
    with pytest.raises(ValueError, match="is not positive definite"):
        ctx.set_prior(np.zeros(3), -np.eye(3), 1.0, 0.02)
