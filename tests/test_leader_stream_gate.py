"""The build-time gate on the leader wave's instruction stream (CPU): check_leader_stream.py must
follow the way an iteration takes through the branches, count instructions and taken branches on
it, and pass on the object as built."""
import importlib.util
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "pybmc_amd", "csrc", "check_leader_stream.py")


def load_gate():
    sys.path.insert(0, os.path.dirname(SCRIPT))
    spec = importlib.util.spec_from_file_location("check_leader_stream", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def listing(body, kernel="_ZN3bmc17gibbs_loop_kernelIdLi1ELi0ELi32ELi1ELb0ELb0ELb1EEEvNS_9GibbsArgsE"):
    """A disassembly of `body` = [(text, index of the branch target or None)], 4 bytes each."""
    out = [f"0000000000001000 <{kernel}>:"]
    for i, (text, tgt) in enumerate(body):
        where = f" <{kernel}+0x{4 * tgt:x}>" if tgt is not None else ""
        out.append(f"\t{text:40s} // {0x1000 + 4 * i:012X}:{where}")
    return out


XOR = "v_xor_b32_dpp v4, v6, v6 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1"
LOOP = [
    ("v_rsq_f64_e32 v[0:1], v[2:3]", None),                    # 0  the draw
    ("s_barrier", None),                                       # 1  B1
    ("v_fmac_f64_dpp v[0:1], v[2:3], -v[4:5] row_newbcast:15 row_mask:0xf bank_mask:0xf", None),  # 2
    ("ds_write_b64 v7, v[0:1]", None),                         # 3
    ("s_cbranch_scc1 21", 23),                                 # 4  the abort word: leaves the loop
    ("s_and_saveexec_b64 s[2:3], s[4:5]", None),               # 5
    ("s_cbranch_execz 7", 8),                                  # 6  never taken: lanes < K exist
    ("global_load_dwordx2 v[8:9], v6, s[8:9]", None),          # 7  xi
    ("global_load_dwordx2 v[10:11], v3, s[10:11] offset:8", None),  # 8  gamma
    ("s_barrier", None),                                       # 9  B2
    ("global_store_dwordx2 v1, v[0:1], s[12:13] sc0", None),   # 10 the granule
    ("global_load_dwordx2 v[12:13], v[14:15], off sc1", None), # 11 poll
    ("v_cmp_eq_u32_e32 vcc, s20, v13", None),                  # 12 tag of read 0
    ("s_cbranch_scc1 16", 17),                                 # 13 hit: taken
    ("v_cmp_eq_u32_e32 vcc, s20, v15", None),                  # 14 tag of read 1
    ("s_cbranch_scc0 11", 11),                                 # 15 miss: round again
    ("s_nop 0", None),                                         # 16
    (XOR, None),                                               # 17 the sum
    ("v_add_f64 v[4:5], v[4:5], s[6:7]", None),                # 18 its last add
    ("s_waitcnt vmcnt(0)", None),                              # 19 the pending poll retired
    ("v_cmp_lt_f64_e32 vcc, v[0:1], v[2:3]", None),            # 20 the floor of the sigma2 step
    ("s_cbranch_scc0 22", 23),                                 # 21 iterations left == 0
    ("s_branch 0", 0),                                         # 22 the back edge
    ("s_endpgm", None),                                        # 23
]


def test_stretches_follow_the_way_an_iteration_takes():
    m = load_gate()
    got = m.measure(m.parse(listing(LOOP)))
    # pass -> B2: 3 .. 8 (the execz branch falls through, the abort branch is not the way to B2)
    assert got["pass -> B2"] == (6, 0)
    assert got["hit 0 -> sum"] == (1, 1)          # 13, taken
    assert got["hit 1 -> sum"] == (2, 0)          # 15, 16
    # sum -> draw: 19, 20, 21, 22 with the back edge taken
    assert got["sum -> draw"] == (4, 1)


def test_only_the_headline_kernel_is_read_and_a_longer_stretch_is_counted():
    m = load_gate()
    other = listing([("s_barrier", None), (XOR, None), ("s_endpgm", None)], kernel="_ZN3bmc5otherEv")
    longer = LOOP[:16] + [("s_nop 0", None), ("s_nop 0", None)] + LOOP[16:]
    longer = [(t, g if g is None or g < 16 else g + 2) for t, g in longer]
    got = m.measure(m.parse(other + listing(longer)))
    assert got["hit 1 -> sum"] == (4, 0) and got["hit 0 -> sum"] == (1, 1)


def test_leader_stream_gate_passes_on_the_built_object():
    obj = os.path.join(ROOT, "pybmc_amd", "csrc", "kernels_gibbs.o")
    if not os.path.exists(obj):      # (objects are build products; build() makes them)
        import pytest
        pytest.skip("kernels_gibbs.o not built")
    r = subprocess.run([sys.executable, SCRIPT, obj], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.startswith("check_leader_stream: pass -> B2 "), r.stdout
