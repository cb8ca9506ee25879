"""The build-time gates on the leader's hit path (CPU): check_leader_stream.py must follow a hit of
the asm gather through the one branch it takes, check_gather_tail.py must flag a write to a
register in which a poll of that gather may still land, and both must pass on the object as
built."""
import importlib.util
import os
import subprocess
import sys

from test_leader_stream_gate import listing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pybmc_amd", "csrc")


def load(name):
    sys.path.insert(0, CSRC)
    spec = importlib.util.spec_from_file_location(name, os.path.join(CSRC, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


XOR = "v_xor_b32_dpp v4, v6, v6 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1"
# the leader's loop with the poll rounds as the asm statement lays them out
LOOP = [
    ("v_rsq_f64_e32 v[0:1], v[2:3]", None),                          # 0  the draw
    ("s_barrier", None),                                             # 1  B1
    ("v_fmac_f64_dpp v[0:1], v[2:3], -v[4:5] row_newbcast:15 row_mask:0xf bank_mask:0xf", None),  # 2
    ("ds_write_b64 v7, v[0:1]", None),                               # 3
    ("s_cbranch_scc1 33", 38),                                       # 4  the abort word: leaves the loop
    ("s_and_saveexec_b64 s[2:3], s[4:5]", None),                     # 5
    ("s_cbranch_execz 7", 8),                                        # 6  never taken
    ("global_load_dwordx2 v[8:9], v6, s[8:9]", None),                # 7  xi
    ("global_load_dwordx2 v[10:11], v3, s[10:11] offset:8", None),   # 8  gamma
    ("s_barrier", None),                                             # 9  B2
    ("global_store_dwordx2 v1, v[0:1], s[12:13] sc0", None),         # 10 the granule
    ("global_load_dwordx2 v[124:125], v[14:15], off sc1", None),     # 11 the statement: first read
    ("global_load_dwordx2 v[126:127], v[14:15], off sc1", None),     # 12 header: second read
    ("s_waitcnt vmcnt(1)", None),                                    # 13
    ("v_cmp_eq_u32_e32 vcc, s20, v125", None),                       # 14 tag of read 0
    ("s_cmp_eq_u64 vcc, -1", None),                                  # 15
    ("s_cbranch_scc0 2", 19),                                        # 16 a hit falls through
    ("v_cndmask_b32_e64 v6, 0, v124, s[8:9]", None),                 # 17 its select
    ("s_branch 11", 30),                                             # 18 ... and takes ONE branch
    ("global_load_dwordx2 v[124:125], v[14:15], off sc1", None),     # 19 read 0 again
    ("s_waitcnt vmcnt(1)", None),                                    # 20
    ("v_cmp_eq_u32_e32 vcc, s20, v127", None),                       # 21 tag of read 1
    ("s_cmp_eq_u64 vcc, -1", None),                                  # 22
    ("s_cbranch_scc1 5", 29),                                        # 23 a hit takes ONE branch
    ("s_add_i32 s21, s21, -1", None),                                # 24 rounds left
    ("s_cmp_lg_u32 s21, 0", None),                                   # 25
    ("s_cbranch_scc1 65521", 12),                                    # 26 round again
    ("v_mov_b32_e32 v6, 0", None),                                   # 27 ran out
    ("s_branch 1", 30),                                              # 28
    ("v_cndmask_b32_e64 v6, 0, v126, s[8:9]", None),                 # 29 the select of read 1
    ("s_cmp_lg_u32 s21, 0", None),                                   # 30 behind the statement
    ("s_cbranch_scc0 6", 38),                                        # 31 ran out: out of line
    (XOR, None),                                                     # 32 the sum
    ("v_add_f64 v[4:5], v[4:5], s[6:7]", None),                      # 33 its last add
    ("s_waitcnt vmcnt(0)", None),                                    # 34 the pending poll retired
    ("v_cmp_lt_f64_e32 vcc, v[0:1], v[2:3]", None),                  # 35 the floor of the sigma2 step
    ("s_cbranch_scc0 1", 38),                                        # 36 iterations left == 0
    ("s_branch 0", 0),                                               # 37 the back edge
    ("s_endpgm", None),                                              # 38
]


def test_a_hit_is_followed_through_the_one_branch_it_takes():
    m = load("check_leader_stream")
    got = m.measure(m.parse(listing(LOOP)))
    assert got["hit 0 -> sum"] == (6, 1)          # 15 16 17 18(taken) 30 31
    assert got["hit 1 -> sum"] == (5, 1)          # 22 23(taken) 29 30 31
    assert got["sum -> draw"] == (4, 1)
    assert m.placement(m.parse(listing(LOOP)))["poll"] == 0x1000 + 4 * 12
    for name in ("hit 0 -> sum", "hit 1 -> sum"):
        assert m.LIMITS[name][1] == 1, (name, m.LIMITS[name])


def test_a_second_branch_on_the_way_of_a_hit_is_counted():
    m = load("check_leader_stream")
    # the select of read 1 moved away from the end of the statement: its hit branches twice
    body = LOOP[:29] + [LOOP[29], ("s_branch 1", 32), ("s_nop 0", None)] + LOOP[30:]
    body = [(t, g if g is None or g < 30 else g + 2) for t, g in body[:31]] + \
           [(t, g if g is None or g < 30 else g + 2) for t, g in body[31:]]
    got = m.measure(m.parse(listing(body)))
    assert got["hit 1 -> sum"][1] == 2, got


DUMP = ["0000 <kernel_a>:"] + ["\t" + t for t, _ in LOOP]


def test_pending_poll_rule_passes_a_clean_listing_and_counts_the_statement():
    m = load("check_gather_tail")
    assert m.scan_polls(DUMP) == (1, [])
    # behind the retiring wait the registers are anybody's
    after = DUMP[:36] + ["\tv_mov_b32_e32 v125, v3"] + DUMP[36:]
    assert m.scan_polls(after) == (1, [])
    # a store that names them as data, and a read of them, write nothing
    reads = DUMP[:34] + ["\tglobal_store_dwordx2 v1, v[126:127], s[12:13]", "\tv_mov_b32_e32 v9, v124"] + DUMP[34:]
    assert m.scan_polls(reads) == (1, [])


def test_pending_poll_rule_flags_a_write_between_the_statement_and_the_wait():
    m = load("check_gather_tail")
    for offender in ("v_mov_b32_e32 v126, v3", "v_add_f64 v[126:127], v[4:5], v[4:5]",
                     "v_mov_b32_dpp v124, v2 row_mirror row_mask:0xf bank_mask:0xf bound_ctrl:1",
                     "global_load_dwordx2 v[124:125], v6, s[8:9]", "ds_read_b64 v[126:127], v7"):
        n, bad = m.scan_polls(DUMP[:34] + ["\t" + offender] + DUMP[34:])
        assert n == 1 and len(bad) == 1 and "kernel_a" in bad[0] and offender.split()[0] in bad[0], (offender, bad)
    # a wait that leaves a read pending does not end the window
    n, bad = m.scan_polls(DUMP[:34] + ["\ts_waitcnt vmcnt(1)", "\tv_mov_b32_e32 v127, v3"] + DUMP[34:])
    assert len(bad) == 1


def test_both_gates_pass_on_the_built_object():
    obj = os.path.join(CSRC, "kernels_gibbs.o")
    if not os.path.exists(obj):      # (objects are build products; build() makes them)
        import pytest
        pytest.skip("kernels_gibbs.o not built")
    r = subprocess.run([sys.executable, os.path.join(CSRC, "check_leader_stream.py"), obj],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "hit 0 -> sum" in r.stdout and "hit 1 -> sum" in r.stdout, r.stdout
    r = subprocess.run([sys.executable, os.path.join(CSRC, "check_gather_tail.py"), obj],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    words = r.stdout.split()
    assert "asm" in words and int(words[words.index("asm") - 1]) > 0, r.stdout
