"""The CPU build of pybmc_amd/csrc/bmc_math.h's Box-Muller transform, for the tests that compare
the device with it bit for bit: g++ compiles tests/rng_host_check.cpp the way
tests/test_host_math.py compiles its program (-O2 -ffp-contract=off), once per session."""
import os
import subprocess
import tempfile

import numpy as np

import rng_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
_dir = None


def _exe():
    global _dir
    if _dir is None:
        _dir = tempfile.TemporaryDirectory(prefix="rng_host_check_")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o", os.path.join(_dir.name, "rng_host_check"),
                        os.path.join(HERE, "rng_host_check.cpp")], check=True)
    return os.path.join(_dir.name, "rng_host_check")


def box_muller(u1, u2):
    """(z0, z1) float64 of bmc::box_muller_pair on float64 arrays of any (equal) shape."""
    exe = _exe()
    u = np.stack([np.asarray(u1, np.float64).ravel(), np.asarray(u2, np.float64).ravel()], axis=1)
    with tempfile.TemporaryDirectory(prefix="rng_host_io_") as d:
        fin, fout = os.path.join(d, "u.bin"), os.path.join(d, "z.bin")
        u.tofile(fin)
        subprocess.run([exe, fin, fout], check=True)
        z = np.fromfile(fout, dtype=np.float64).reshape(-1, 2)
    assert z.shape == u.shape
    return z[:, 0].reshape(np.shape(u1)), z[:, 1].reshape(np.shape(u1))


def normals(seed, n):
    """The normal stream through the CPU build: what the header promises the device computes."""
    return R.interleave(*box_muller(*R.normal_pair_uniforms(seed, n)), n)


def predict_noise(seed, n_draws, n_points):
    u1, u2, half = R.predict_noise_uniforms(seed, n_draws, n_points)
    z0, z1 = box_muller(u1, u2)
    return np.where(half[None, :] == 1, z1, z0)
