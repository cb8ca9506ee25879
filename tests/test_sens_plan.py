"""The host plan of the power-scaling sensitivity on the CPU: g++ builds tests/sens_plan_check.cpp
from the header the library is built from (bmc_sens_plan.h: limits, tail length, sort segment,
scan chunks, batches, scratch sizes), plain and with -fsanitize=address,undefined as a stand-alone
program; and the argument checks of pybmc_amd.sensitivity that need no GPU."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import sens_reference as SR
from psis_reference import tail_length

HERE = os.path.dirname(os.path.abspath(__file__))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]


def build_plan_check(tmp, extra=()):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is required")
    exe = tmp / "sens_plan_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *extra,
                        os.path.join(HERE, "sens_plan_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def run_plan_check(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


def fields(line):
    return dict(kv.split("=", 1) for kv in line.split() if "=" in kv)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    return build_plan_check(tmp_path_factory.mktemp("sens_" + request.param),
                            SAN if request.param == "sanitized" else ())


def test_sweep_of_shapes_batches_and_budgets(exe):
    word, plans, failures = run_plan_check(exe, "sweep").split()
    assert word == "sweep" and int(plans) > 10000 and int(failures) == 0


def test_tail_length_is_the_reference_rule(exe):
    for S in (1, 4, 24, 25, 224, 225, 226, 227, 2047, 2048, 4096, 4101, 50000, 3200000):
        f = fields(run_plan_check(exe, "tail", S))
        M = tail_length(S)
        assert int(f["M"]) == M
        assert int(f["grid"]) == (30 + int(math.floor(math.sqrt(M))) if M >= 5 else 0)


def _ceil_isqrt(v):
    """numpy int64 ceil(sqrt(v)), v < 2^62: the float root, put right in integers"""
    r = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
    r -= r * r > v
    r += (r + 1) * (r + 1) <= v
    assert np.all((r * r <= v) & ((r + 1) * (r + 1) > v))
    return r + (r * r < v)


def test_the_one_tail_rule_in_integers(exe):
    """psis_tail_length and psis_grid_points (bmc_psis_plan.h) against M = min(S // 5,
    ceil_isqrt(9 S)) and grid = 30 + isqrt(M) in integers: every S up to 2^23, five values around
    every 9 S = r^2 up to r = 139000, and the ends of the 32-bit range; and plan_loo's tail is 0
    exactly when M < 5, M otherwise."""
    r = np.arange(3, 139001, dtype=np.int64)
    near = ((r * r) // 9)[:, None] + np.arange(-2, 3, dtype=np.int64)
    S = np.concatenate([np.arange(1, 2 ** 23 + 1, dtype=np.int64), near.reshape(-1),
                        np.array([2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2], dtype=np.int64)])
    S = S[S >= 1]
    p = subprocess.run([exe, "tails"], input=S.tobytes(), capture_output=True)
    assert p.returncode == 0, p.stderr[-2000:]
    M, grid, loo_tail = np.frombuffer(p.stdout, dtype=np.int32).reshape(-1, 3).astype(np.int64).T
    assert len(M) == len(S)
    want = np.minimum(S // 5, _ceil_isqrt(9 * S))
    bad = np.flatnonzero(M != want)
    assert bad.size == 0, (S[bad[:5]], M[bad[:5]], want[bad[:5]])
    assert np.array_equal(grid, 30 + (_ceil_isqrt(M + 1) - 1))      # floor(sqrt(M)) = ceil(sqrt(M + 1)) - 1
    assert np.array_equal(loo_tail, np.where(M < 5, 0, M))
    assert np.array_equal(loo_tail == 0, M < 5) and (M < 5).any() and (M >= 5).any()
    for s in (1, 24, 25, 224, 225, 226, 2 ** 23, 139000 ** 2 // 9, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2):
        i = int(np.flatnonzero(S == s)[0])                          # and math.isqrt itself on a few
        m = min(s // 5, math.isqrt(9 * s - 1) + 1)
        assert (M[i], grid[i]) == (m, 30 + math.isqrt(m)), s


def test_plan_of_the_benchmark_shape(exe):
    f = fields(run_plan_check(exe, "plan", 3200000, 33, 4, 0, 100 * 2 ** 30))
    assert f["ok"] == "1" and f["n_batches"] == "1" and f["cols_per_batch"] == "33"
    assert int(f["chunks"]) == -(-3200000 // 2048) and int(f["tiles"]) == -(-3200000 // 4096)
    g = fields(run_plan_check(exe, "plan", 3200001, 33, 4, 5, 0))
    assert g["ok"] == "1" and g["S_pad"] == "3200002" and g["n_batches"] == "7"
    h = fields(run_plan_check(exe, "plan", 3200000, 33, 4, 0, 1000))
    assert h["ok"] == "0"


def test_argument_refusals(exe):
    ok = (10, 3, 100, 2, 1, 1.01, 3)
    assert run_plan_check(exe, "check", *ok).strip() == "ok"
    for pos, bad in ((0, 0), (1, 0), (1, 257), (2, 1), (2, 2 ** 31 - 1), (3, -1), (3, 4097), (4, 0),
                     (5, 1.0), (5, 0.0), (5, -2.0), (5, "nan"), (5, "inf"), (6, 0), (6, 16)):
        args = list(ok)
        args[pos] = bad
        assert run_plan_check(exe, "check", *args).strip() != "ok", (pos, bad)


# ---- the Python argument checks (they raise before a context is made) ----------------------------
def _case():
    return SR.random_case(12, 2, 40, 1, n_models=2)


@pytest.mark.parametrize("kwargs", [
    {"alphas": [0.5, 1.0]}, {"alphas": [0.0]}, {"alphas": [-1.0]}, {"alphas": [np.nan]},
    {"alphas": np.linspace(1.1, 2, 65)}, {"alpha_lo": 1.0}, {"alpha_hi": 0.5},
    {"components": ("prior", "posterior")}, {"components": ()}, {"components": ("prior", "prior")},
])
def test_bad_arguments_raise_value_error(kwargs):
    from pybmc_amd.sensitivity import power_scale_sensitivity
    A, y, theta, prior, Vt = _case()
    with pytest.raises(ValueError):
        power_scale_sensitivity(A, y, theta, prior, Vt, **kwargs)


def test_shapes_that_do_not_agree_raise_value_error():
    from pybmc_amd.sensitivity import power_scale_sensitivity, power_scale_weights
    A, y, theta, prior, Vt = _case()
    b0, C0, nu0, s20 = prior
    for bad in ([b0[:1], C0, nu0, s20], [b0, C0[:1], nu0, s20], [b0, C0, -1.0, s20], [b0, C0, nu0]):
        with pytest.raises(ValueError):
            power_scale_sensitivity(A, y, theta, bad)
    with pytest.raises(ValueError):
        power_scale_sensitivity(A, y, theta, prior, Vt[:1])
    with pytest.raises(ValueError):
        power_scale_sensitivity(A, y[:-1], theta, prior)
    with pytest.raises(ValueError):
        power_scale_sensitivity(A, y, theta[:, :-1], prior)
    with pytest.raises(ValueError):
        power_scale_weights(A, y, theta, prior, component="evidence")
    with pytest.raises(ValueError):
        power_scale_weights(A, y, theta, prior, alpha=1.0)


def test_names_are_exported():
    import pybmc_amd
    for name in ("power_scale_sensitivity", "power_scale_weights", "sensitivity_summary"):
        assert name in pybmc_amd.__all__ and callable(getattr(pybmc_amd, name))
    assert callable(pybmc_amd.BayesianModelCombination.prior_sensitivity)


def test_summary_table_and_diagnosis():
    from pybmc_amd.sensitivity import CONFLICT, NO_FINDING, STRONG_PRIOR, diagnose, sensitivity_summary
    assert diagnose(0.05, 0.05) == CONFLICT and diagnose(0.2, 0.049) == STRONG_PRIOR
    assert diagnose(0.049, 0.3) == NO_FINDING and diagnose(float("nan"), 0.3) == NO_FINDING
    res = {"columns": ["beta_0", "sigma"], "components": ("prior", "likelihood"),
           "psens": {"prior": np.array([0.2, 0.01]), "likelihood": np.array([0.1, 0.3])}}
    t = sensitivity_summary(res)
    assert list(t.index) == ["beta_0", "sigma"] and list(t.columns) == ["prior", "likelihood", "diagnosis"]
    assert list(t["diagnosis"]) == [CONFLICT, NO_FINDING]
    assert list(sensitivity_summary(res, threshold=0.15)["diagnosis"]) == [STRONG_PRIOR, NO_FINDING]
