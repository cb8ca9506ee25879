"""The CPU build of pybmc_amd/csrc/bmc_math.h's Student-t distribution function, for the tests that
hold it to mpmath and compare the device's values with it: g++ compiles
tests/loo_predict_t_math_check.cpp the way tests/predict_t_host_build.py compiles its program
(-O2 -ffp-contract=off), once per session."""
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_dir = None


def _exe():
    global _dir
    if _dir is None:
        _dir = tempfile.TemporaryDirectory(prefix="loo_predict_t_math_check_")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o",
                        os.path.join(_dir.name, "loo_predict_t_math_check"),
                        os.path.join(HERE, "loo_predict_t_math_check.cpp")], check=True)
    return os.path.join(_dir.name, "loo_predict_t_math_check")


def limits():
    """(nu_min, nu_max, max_steps) of bmc_math.h."""
    r = subprocess.run([_exe(), "limits"], check=True, capture_output=True, text=True).stdout.split()
    return float(r[0]), float(r[1]), int(r[2])


def t_cdf(z, nu):
    """(F, steps, f) float64 arrays of z's shape: bmc::student_t_cdf(z, nu, f) with the density f the
    scoring kernels form, and the continued fraction's steps (nu is broadcast to z)."""
    z = np.asarray(z, np.float64)
    pairs = np.stack([z.ravel(), np.broadcast_to(np.asarray(nu, np.float64), z.shape).ravel()], axis=1)
    with tempfile.TemporaryDirectory(prefix="loo_predict_t_io_") as d:
        fin, fout = os.path.join(d, "z.bin"), os.path.join(d, "F.bin")
        pairs.tofile(fin)
        subprocess.run([_exe(), fin, fout], check=True)
        out = np.fromfile(fout, dtype=np.float64).reshape(-1, 3)
    assert out.shape[0] == pairs.shape[0]
    return tuple(out[:, j].reshape(z.shape) for j in range(3))
