"""The CPU build of pybmc_amd/csrc/bmc_math.h's Student-t variate, for the tests that compare the
predictive kernel's t noise with it bit for bit: g++ compiles tests/predict_t_math_check.cpp the way
tests/rng_host_build.py compiles its program (-O2 -ffp-contract=off), once per session."""
import os
import subprocess
import tempfile

import numpy as np

import predict_t_reference as PT

HERE = os.path.dirname(os.path.abspath(__file__))
_dir = None


def _exe():
    global _dir
    if _dir is None:
        _dir = tempfile.TemporaryDirectory(prefix="predict_t_math_check_")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o",
                        os.path.join(_dir.name, "predict_t_math_check"),
                        os.path.join(HERE, "predict_t_math_check.cpp")], check=True)
    return os.path.join(_dir.name, "predict_t_math_check")


def t_variate(u1, u2, nu):
    """float64 bmc::student_t_variate(u1, u2, nu, 2 / nu) on float64 arrays of one shape (nu is
    broadcast to it)."""
    exe = _exe()
    u1 = np.asarray(u1, np.float64)
    tri = np.stack([u1.ravel(), np.asarray(u2, np.float64).ravel(),
                    np.broadcast_to(np.asarray(nu, np.float64), u1.shape).ravel()], axis=1)
    with tempfile.TemporaryDirectory(prefix="predict_t_io_") as d:
        fin, fout = os.path.join(d, "u.bin"), os.path.join(d, "t.bin")
        tri.tofile(fin)
        subprocess.run([exe, fin, fout], check=True)
        t = np.fromfile(fout, dtype=np.float64)
    assert t.shape == (tri.shape[0],)
    return t.reshape(u1.shape)


def noise(seed, S, M, nu):
    """(S, M) float64: the predictive t noise through the CPU build -- what the device is to compute."""
    u1, u2 = PT.uniforms(seed, S, M)
    return t_variate(u1, u2, PT.nu_of_draws(nu, S)[:, None])
