"""The gate's stretches behind barrier B1 (CPU): check_leader_stream.py must count what stands
between the barrier and the LDS read of the u rows (nothing may), and between the barrier and the
first DPP FMA of the residual pass; both have limits, and the object as built passes them."""
import os
import subprocess
import sys

from test_leader_stream_gate import LOOP, ROOT, SCRIPT, listing, load_gate

U_READ = ("ds_read2_b64 v[96:99], v104 offset1:16", None)
COPY = ("v_mov_b64_e32 v[100:101], 0", None)
WAIT = ("s_waitcnt lgkmcnt(0)", None)


def behind_b1(extra):
    """LOOP with `extra` instructions between barrier B1 (index 1) and the first FMA (index 2)."""
    body = LOOP[:2] + extra + LOOP[2:]
    n = len(extra)
    return [(t, g if g is None or g < 2 else g + n) for t, g in body]


def test_u_read_first_behind_the_barrier_counts_zero():
    m = load_gate()
    got = m.measure(m.parse(listing(behind_b1([U_READ, COPY, COPY, WAIT]))))
    assert got["B1 -> u"] == (0, 0)
    assert got["B1 -> pass"] == (4, 0)
    assert got["pass -> B2"] == (6, 0)         # (the stretches behind the pass are where they were)
    assert got["sum -> draw"] == (4, 1)


def test_copies_in_front_of_the_u_read_are_counted():
    m = load_gate()
    got = m.measure(m.parse(listing(behind_b1([COPY, COPY, U_READ, WAIT]))))
    assert got["B1 -> u"] == (2, 0)
    assert got["B1 -> pass"] == (4, 0)


def test_both_stretches_have_limits_and_the_u_read_stands_first():
    m = load_gate()
    assert m.LIMITS["B1 -> u"] == (0, 0)
    assert "B1 -> pass" in m.LIMITS
    got = m.measure(m.parse(listing(behind_b1([U_READ, WAIT]))))
    assert set(got) <= set(m.LIMITS)           # (every stretch that is reported has a limit)


def test_gate_reports_the_b1_stretches_on_the_built_object():
    obj = os.path.join(ROOT, "pybmc_amd", "csrc", "kernels_gibbs.o")
    if not os.path.exists(obj):      # (objects are build products; build() makes them)
        import pytest
        pytest.skip("kernels_gibbs.o not built")
    r = subprocess.run([sys.executable, SCRIPT, obj], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "B1 -> u 0 instructions 0 taken" in r.stdout, r.stdout
    assert "B1 -> pass " in r.stdout, r.stdout
