"""The cases of tests/test_row_sum_classes_gpu.py and scripts/record_row_sum_golden.py: every wave
count of the leader's row sum (a group of nw waves leaves nw rows of lane partials, the other rows
stay zero), with a ragged last panel and with an absent panel whose zero row lies among the rows
of waves that exist; the residual pass with two and four column blocks; the agent-scope copy of
the headline geometry; two chains with streams of their own.

All cases run in replay mode on the seeded streams of leader_stream_cases: the chains are compared
with the bits of the commit the goldens were recorded at (the parent of the change that moved the
u read behind barrier B1 and shortened the leader's wave sum), not with the oracle.  One module builds the inputs for the recorder and for the
test, so that a golden and the run compared with it start from the same bits.

A golden is tests/golden/row_sum/<name>.npy: ONE chain [T, k + 1]; the pair case keeps both chains
of its launch, [2, T, k + 1].

Case table (n rows -> ceil(n / 64) panels of 64 rows, dealt to the G groups in turn; one panel per
wave).  The planner reaches every geometry asked for, so no n had to be moved:

  k16_w{w}_full    n = 128 w - 7,  G = 2: both groups have w panels, the last one ragged (57 rows)
  k16_w{w}_absent  n = 128 w - 71, G = 2 (w >= 2): group 1 has w - 1 panels, its wave w - 1 none
  k32_w3           n = 377, k = 32, G = 2, w = 3: two column blocks
  k64_g3           n = 640, k = 64, G = 3 (4 waves, the planner's): four column blocks
  headline_agent   n = 10 000, k = 32, G = 32, w = 5, agent scope forced, T = 65
  pair_w5          n = 633, k = 16, G = 2, w = 5: two chains, chain 0 must equal its solo run
"""
import os

import leader_stream_cases as lc

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "row_sum")
HEADLINE_KERNEL = "gibbs_loop_kernel<double, 1, 0, 32, 1, false, false, true>"

# name: (n, k, tuning keywords, T, what the launch must report)
CASES = {}
for _w in range(1, 9):
    _t = dict(groups_per_chain=2, waves_per_group=_w)
    CASES[f"k16_w{_w}_full"] = (128 * _w - 7, 16, _t, 3, _t)
    if _w >= 2:
        CASES[f"k16_w{_w}_absent"] = (128 * _w - 71, 16, _t, 3, _t)
CASES["k32_w3"] = (377, 32, dict(groups_per_chain=2, waves_per_group=3), 3,
                   dict(groups_per_chain=2, waves_per_group=3))
CASES["k64_g3"] = (640, 64, dict(groups_per_chain=3), 3, dict(groups_per_chain=3, waves_per_group=4))
HEADLINE_AGENT = "headline_agent"
CASES[HEADLINE_AGENT] = (10000, 32, dict(force_agent_scope=1), 65,
                         dict(groups_per_chain=32, waves_per_group=5, xcd_local_chains=0))
PAIR = "pair_w5"
PAIR_SHAPE = (633, 16, 3)          # n, k, T
PAIR_TUNING = dict(groups_per_chain=2, waves_per_group=5)


def golden_path(name):
    return os.path.join(GOLDEN_DIR, name + ".npy")


def run_case(ctx, name):
    """Returns (chain [T, k + 1], stats); asserts that the launch had the geometry asked for."""
    n, k, tuning, T, want = CASES[name]
    lc.load(ctx, n, k)
    ctx.set_tuning(**tuning)
    try:
        out, st = lc.run_replay(ctx, n, k, T)
    finally:
        ctx.set_tuning()
    lc.check_stats(name, st, want)
    return out[0], st


def run_pair(ctx):
    """Two chains with streams of their own in one launch at five waves, and chain 0 alone.
    Returns (pair [2, T, k + 1], alone [T, k + 1], stats)."""
    n, k, T = PAIR_SHAPE
    lc.load(ctx, n, k)
    ctx.set_tuning(**PAIR_TUNING)
    try:
        pair, st = lc.run_replay(ctx, n, k, T, (0, 1))
        alone, st1 = lc.run_replay(ctx, n, k, T, (0,))
    finally:
        ctx.set_tuning()
    for s in (st, st1):
        lc.check_stats(PAIR, s, PAIR_TUNING)
    assert st["n_chains"] == 2 and st["launches"] == 1, st
    return pair, alone[0], st
