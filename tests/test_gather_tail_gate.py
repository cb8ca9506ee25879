"""The build-time gate on the group sum behind a granule gather (CPU): check_gather_tail.py must
flag a wait on vmcnt inside the sum, name the kernel, and let every other wait pass."""
import importlib.util
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "pybmc_amd", "csrc", "check_gather_tail.py")


def load_scanner():
    spec = importlib.util.spec_from_file_location("check_gather_tail", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


XOR = "\tv_xor_b32_dpp v100, v104, v%d quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1"
HEAD = ["0000 <kernel_a>:", "\tglobal_load_dwordx2 v[102:103], v[100:101], off sc1", "\ts_waitcnt vmcnt(1)",
        XOR % 104, "\tv_cndmask_b32_e64 v100, v100, 0, s[10:11]", "\tv_xor_b32_e32 v101, v100, v104",
        "\ts_nop 0", XOR % 100]
STEP = ["\tv_mov_b32_dpp v107, v101 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1",
        "\tv_mov_b32_dpp v106, v100 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1",
        "\tv_add_f64 v[100:101], v[106:107], v[100:101]"]
READS = ["\tv_readlane_b32 s%d, v%d, %d" % (12 + 2 * i + h, 101 - h, 16 * i) for i in range(4) for h in range(2)]
TAIL = ["\tv_add_f64 v[100:101], s[12:13], v[106:107]", "\ts_waitcnt vmcnt(0)", "\ts_endpgm"]


def test_scanner_passes_a_clean_sum_and_counts_it():
    m = load_scanner()
    n, exempt, bad = m.scan(HEAD + STEP + READS + TAIL)
    # (the xor swap's second half opens no second window; the wait behind the last lane read and
    # the one in front of the first xor are outside it)
    assert (n, exempt, bad) == (1, 0, [])
    n, exempt, bad = m.scan(HEAD + STEP + READS + TAIL + ["0100 <kernel_b>:"] + HEAD[1:] + STEP + READS + TAIL)
    assert (n, exempt, bad) == (2, 0, [])


def test_scanner_flags_a_vmcnt_wait_inside_the_sum_with_the_kernel_name():
    m = load_scanner()
    n, exempt, bad = m.scan(HEAD + ["\ts_waitcnt vmcnt(0)"] + STEP + READS + TAIL)
    assert n == 1 and len(bad) == 1 and "kernel_a" in bad[0] and "vmcnt(0)" in bad[0]
    # between the lane reads, and combined with another counter: still a wait on vmcnt
    n, exempt, bad = m.scan(HEAD + STEP + READS[:3] + ["\ts_waitcnt vmcnt(0) lgkmcnt(0)"] + READS[3:] + TAIL)
    assert len(bad) == 1 and "3 of 8" in bad[0]
    # the second kernel of a listing is named as itself
    n, exempt, bad = m.scan(HEAD + STEP + READS + TAIL + ["0100 <kernel_b>:"] + HEAD[1:] + STEP
                            + ["\ts_waitcnt vmcnt(1)"] + READS + TAIL)
    assert n == 2 and len(bad) == 1 and "kernel_b" in bad[0]


def test_scanner_lets_an_lgkmcnt_wait_pass():
    m = load_scanner()
    n, exempt, bad = m.scan(HEAD + ["\ts_waitcnt lgkmcnt(0)"] + STEP + READS + TAIL)
    assert (n, exempt, bad) == (1, 0, [])


def test_gather_tail_gate_passes_on_the_built_objects():
    obj = os.path.join(ROOT, "pybmc_amd", "csrc", "kernels_gibbs.o")
    if not os.path.exists(obj):      # (objects are build products; build() makes them)
        import pytest
        pytest.skip("kernels_gibbs.o not built")
    r = subprocess.run([sys.executable, SCRIPT, obj], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    words = r.stdout.split()
    assert words[0] == "check_gather_tail:" and int(words[1]) > 0, r.stdout
