"""The host side of the Student-t forms of the power-scaling sensitivity on the CPU: g++ builds
tests/sens_t_plan_check.cpp from the headers the library is built from (bmc_sens_plan.h: the
validator of the five component bits and of the nu table, the plan at the wider weight-vector
bound; bmc_math.h: a padded point adds exactly 0), plain and with -fsanitize=address,undefined as a
stand-alone program."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is required")
    out = tmp_path_factory.mktemp("sens_t_" + request.param) / "sens_t_plan_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror",
                        *(SAN if request.param == "sanitized" else ()),
                        os.path.join(HERE, "sens_t_plan_check.cpp"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(out)


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout.strip()


def fields(line):
    return dict(kv.split("=", 1) for kv in line.split() if "=" in kv)


def test_constants(exe):
    f = fields(run(exe, "const"))
    assert f == {"components": "5", "gaussian_components": "4", "logdens": "4", "max_nu_values": "4096",
                 "max_w": "340", "gaussian_max_w": "264"}


def test_a_padded_point_adds_exactly_zero(exe):
    assert run(exe, "zero") == "zero 0"


def test_the_plan_is_the_gaussian_one_up_to_its_bound_and_goes_on_to_340(exe):
    word, plans, failures = run(exe, "sweep").split()
    assert word == "sweep" and int(plans) > 5000 and int(failures) == 0
    # five components x 66 alphas, the estimated-nu columns of the benchmark shape
    f = fields(run(exe, "plan", 3200000, 34, 330, 0, 100 * 2 ** 30))
    assert f["ok"] == "1" and f["W"] == "330" and f["n_batches"] == "1" and f["cols_per_batch"] == "34"
    chunks = -(-3200000 // 2048)
    assert int(f["part"]) == 34 * 330 * chunks * 6 * 8 and int(f["offs"]) == 34 * 330 * chunks * 8
    assert fields(run(exe, "plan", 100, 4, 341, 0, 2 ** 30))["ok"] == "0"
    assert "340" in run(exe, "plan", 100, 4, 341, 0, 2 ** 30)


# n, k, S, n_models, n_alphas, alpha, components, per_draw, n_values, nu, log prior
OK_FIXED = (10, 3, 100, 2, 1, 1.01, 3, 0, 1, 4.0, "none")
OK_TABLE = (10, 3, 100, 2, 66, 1.01, 31, 1, 7, 4.0, -1.5)


def test_argument_refusals(exe):
    assert run(exe, "check", *OK_FIXED) == "ok" and run(exe, "check", *OK_TABLE) == "ok"
    # the shape and the alphas by the Gaussian form's rules, with its messages
    for pos, bad in ((0, 0), (1, 0), (1, 257), (2, 1), (2, 2 ** 31 - 1), (3, -1), (3, 4097), (4, 0), (4, 67),
                     (5, 1.0), (5, 0.0), (5, "nan"), (5, "inf")):
        for ok in (OK_FIXED, OK_TABLE):
            args = list(ok)
            args[pos] = bad
            assert run(exe, "check", *args) != "ok", (pos, bad)
    # the mask: five bits, the fifth only with a prior of nu
    for ok, bad_masks in ((OK_FIXED, (0, 16, 17, 32)), (OK_TABLE, (0, 32, 63))):
        for m in bad_masks:
            args = list(ok)
            args[6] = m
            assert run(exe, "check", *args) != "ok", m
    no_prior = list(OK_TABLE)
    no_prior[10] = "none"
    assert "prior_nu" in run(exe, "check", *no_prior)
    no_prior[6] = 15
    assert run(exe, "check", *no_prior) == "ok"
    # nu and the table
    for bad in (0.0, -1.0, "nan", "inf"):
        args = list(OK_FIXED)
        args[9] = bad
        assert run(exe, "check", *args) == "nu must be positive and finite"
        args = list(OK_TABLE)
        args[9] = bad
        assert run(exe, "check", *args) == "nu_values must be positive and finite"
    for bad in (0, -1, 4097):
        args = list(OK_TABLE)
        args[8] = bad
        assert run(exe, "check", *args) == "n_values must be between 1 and 4096"
    args = list(OK_TABLE)
    args[8] = 4096
    assert run(exe, "check", *args) == "ok"
    for bad in ("nan", "inf", "-inf"):
        args = list(OK_TABLE)
        args[10] = bad
        assert run(exe, "check", *args) == "nu_log_prior must be finite"


def test_the_gaussian_validator_is_untouched(exe):
    """SENS_COMPONENTS stays 4: bit 4 is refused by sens_check (tests/test_sens_plan.py holds the rest)."""
    text = open(os.path.join(os.path.dirname(HERE), "pybmc_amd", "csrc", "bmc_sens_plan.h")).read()
    assert "constexpr int SENS_COMPONENTS = 4;" in text and "constexpr int SENS_T_COMPONENTS = 5;" in text
    assert '"need between 1 and 264 weight vectors"' in text
