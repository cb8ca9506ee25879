"""The leader-stream gate's stretch from the draw to barrier B1, its reading of a rotated loop and
its placement check (CPU), on synthetic listings in the style of tests/test_leader_stream_gate.py."""
from test_leader_stream_gate import LOOP, XOR, listing, load_gate

# The loop as hipcc lays it out once the leader has a second exit: the sigma2 step stands at the loop
# top, behind the back edge, and the draw hands the recorder nothing in front of B1.
ROTATED = [
    ("s_branch 4", 4),                                         # 0  entry: round the sigma2 step
    ("v_cmp_lt_f64_e32 vcc, v[0:1], v[2:3]", None),            # 1  the floor of the sigma2 step (loop top)
    ("v_cndmask_b32_e32 v3, v3, v8, vcc", None),               # 2
    ("s_cbranch_vccz 27", 27),                                 # 3  iterations left == 0
    ("v_fma_f64 v[0:1], v[2:3], v[4:5], v[6:7]", None),        # 4
    ("v_rsq_f64_e32 v[0:1], v[2:3]", None),                    # 5  the draw
    ("v_mul_f64 v[0:1], v[0:1], v[2:3]", None),                # 6
    ("ds_write_b64 v7, v[0:1]", None),                         # 7  u
    ("s_waitcnt lgkmcnt(0)", None),                            # 8
    ("s_barrier", None),                                       # 9  B1
    ("v_fmac_f64_dpp v[0:1], v[2:3], -v[4:5] row_newbcast:15 row_mask:0xf bank_mask:0xf", None),  # 10
    ("ds_write_b64 v7, v[0:1]", None),                         # 11
    ("global_load_dwordx2 v[10:11], v3, s[10:11] offset:8", None),  # 12 gamma
    ("s_barrier", None),                                       # 13 B2
    ("global_store_dwordx2 v1, v[0:1], s[12:13] sc0", None),   # 14 the granule
    ("ds_write2_b64 v1, v[2:3], v[4:5] offset1:3", None),      # 15 the (sp, g) words, in the idle slot
    ("global_load_dwordx2 v[12:13], v[14:15], off sc1", None), # 16 poll: the poll loop's header
    ("v_cmp_eq_u32_e32 vcc, s20, v13", None),                  # 17 tag of read 0
    ("s_cbranch_scc1 21", 21),                                 # 18 hit: taken
    ("v_cmp_eq_u32_e32 vcc, s20, v15", None),                  # 19 tag of read 1
    ("s_cbranch_scc0 16", 16),                                 # 20 miss: round again
    (XOR, None),                                               # 21 the sum
    ("v_add_f64 v[4:5], v[4:5], s[6:7]", None),                # 22 its last add
    ("s_waitcnt vmcnt(0)", None),                              # 23 the pending poll retired
    ("s_cbranch_scc0 26", 26),                                 # 24 the flag: expired, out of line
    ("s_cbranch_execnz 1", 1),                                 # 25 the back edge
    ("s_branch 1", 1),                                         # 26 the expired block
    ("s_endpgm", None),                                        # 27
]


def test_draw_to_b1_is_counted_on_the_straight_loop():
    m = load_gate()
    got = m.measure(m.parse(listing(LOOP)))
    assert got["draw -> B1"] == (0, 0)                 # the barrier follows the v_rsq_f64 at once
    # three LDS writes of a recorder's pair in front of B1 are three instructions more
    pair = [("s_and_saveexec_b64 s[2:3], s[4:5]", None), ("ds_write_b64 v1, v[2:3]", None),
            ("s_or_b64 exec, exec, s[2:3]", None)]
    longer = LOOP[:1] + pair + LOOP[1:]
    longer = [(t, g if g is None or g < 1 else g + 3) for t, g in longer]
    got = m.measure(m.parse(listing(longer)))
    assert got["draw -> B1"] == (3, 0)
    assert got["pass -> B2"] == (6, 0)                 # (the other stretches are where they were)


def test_rotated_loop_with_the_sigma2_step_at_its_top():
    m = load_gate()
    ins = m.parse(listing(ROTATED))
    assert m.leader_loop(ins) == (1, 25)
    got = m.measure(ins)
    assert got["draw -> B1"] == (3, 0)                 # 6, 7, 8
    assert got["pass -> B2"] == (2, 0)                 # 11, 12
    assert got["hit 0 -> sum"] == (1, 1) and got["hit 1 -> sum"] == (1, 0)
    # sum -> draw: 23, 24, 25 (taken), then the loop top 1, 2, 3, 4
    assert got["sum -> draw"] == (7, 1)


def test_placement_reports_both_headers():
    m = load_gate()
    where = m.placement(m.parse(listing(ROTATED)))     # 4 bytes per instruction from 0x1000
    assert where == {"loop": 0x1000 + 4 * 1, "poll": 0x1000 + 4 * 16}
    where = m.placement(m.parse(listing(LOOP)))
    assert where == {"loop": 0x1000, "poll": 0x1000 + 4 * 11}
    assert m.placement(m.parse(listing([("s_endpgm", None)]))) == {"loop": None, "poll": None}
