#!/usr/bin/env python3
"""Build-time gate: the leader wave's instruction stream in the headline Gibbs kernel stays short.

One iteration of ``gibbs_loop_kernel<double, 1, REG, 32, 1, false, false, SMALLG>`` (one f64 chain
at N = 10 000, K = 32) is a chain of dependent steps of wave 0 of each group, and between the
long steps -- the residual pass, the gather, the group sum, the draw -- every scalar instruction
and every taken branch of that wave is on the serial path.  This script disassembles
the gfx950 code object of the given host object, finds the kernel's loop copy of the leader that
does not record and exchanges at workgroup scope, and counts instructions and taken branches on
these stretches of the way a hit takes:

  draw -> B1     behind the first ``v_rsq_f64`` of the draw, up to the barrier that hands u over
  B1 -> u        behind barrier B1, up to the LDS read of the u rows: nothing stands there (every
                 wave waits out that read's latency, so whatever precedes it delays the pass)
  B1 -> pass     behind barrier B1, up to the first ``v_fmac_f64_dpp`` of the residual pass
  pass -> B2     behind the last ``v_fmac_f64_dpp`` of the residual pass, up to the group barrier
  B2 -> publish  behind the group barrier, up to the store of the group total's granule
  hit N -> sum   behind the tag compare of read N of the gather, up to the first DPP step of the sum
  sum -> draw    behind the last add of the group sum (the one in front of the wait that retires the
                 pending polls), over the loop's back edge, up to the first ``v_rsq_f64`` of the draw

A stretch is the shortest way through the branches from its first to its last instruction, both
excluded; the wave's lane masks are never empty there, so ``s_cbranch_execz`` falls through and
``s_cbranch_execnz`` is taken.  So that the shortest way is the one an iteration really takes, and
not a way round the work, pass -> B2 goes through the load of the next Gamma variate (the last load
in front of the barrier) and sum -> draw through the ``v_cmp_lt_f64`` of the sigma2 step's floor.  The build fails when a count exceeds its value in LIMITS, which
are the counts of the commit that last shortened the stream: a change that lengthens a stretch has
to say so by raising its limit.

Placement.  The same loop, instruction for instruction, runs an iteration 3 % faster or slower with
where its code lies: a sweep of 0 .. 15 ``s_nop`` in front of the loop copies (``BMC_PLACE_PAD``,
kernels_gibbs.hip) has a period of 8, i.e. 32 bytes, best with the iteration loop's header at byte 0
of a 32-byte window.  The poll loop's header is aligned to byte 0 by the asm statement
that holds it, and the padding now stands behind a 32-byte boundary in front of the leader's loop, so
neither header moves with the code above it.  The script prints the two headers'
byte addresses modulo 64 and fails when they are not at PLACE modulo PLACE_PERIOD: a change that
moves the loop has to move it back with ``BMC_PLACE_PAD``, or measure again and say so here.
Usage: check_leader_stream.py [--no-placement] <kernels_gibbs.o>
"""
import heapq
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_dpp_hazard import device_asm  # noqa: E402

KERNEL = "gibbs_loop_kernelIdLi1ELi0ELi32ELi1ELb0ELb0ELb1E"
SUM_HEAD = "quad_perm:[1,0,3,2]"       # v_xor_b32_dpp with it: the first instruction of granule_sum1

# stretch: (instructions, taken branches) at this commit
# (sum -> draw went from 21 to 23 when pass -> B2 went from 20 to 12: the two scalar adds of the xi
# pointer moved from in front of B2 to the loop top, where hipcc now also merges the expired flag
# into the loop's exit condition and no longer needs the move and the branch round the exit block)
LIMITS = {
    "draw -> B1": (20, 0),
    "B1 -> u": (0, 0),
    "B1 -> pass": (7, 0),
    "pass -> B2": (12, 0),
    "B2 -> publish": (53, 0),
    # (the poll rounds are one asm statement, granule_gather1_asm: a hit on read 0 falls into its
    # select and takes one branch to the statement's end, a hit on read 1 takes one branch to its
    # select; behind the statement stand the compare and the branch of "ran out", not taken)
    "hit 0 -> sum": (6, 1),
    "hit 1 -> sum": (5, 1),
    "sum -> draw": (23, 1),
}
# header: byte address modulo PLACE_PERIOD the measured placement has it at
PLACE_PERIOD = 32
PLACE = {"loop": 0, "poll": 0}


def parse(lines, kernel=KERNEL):
    """The kernel's instructions as [mnemonic, text, index of the branch target or None, byte address]."""
    ins, addr_of, on = [], [], False
    for raw in lines:
        line = raw.rstrip("\n")
        if not line.startswith(("\t", " ")):
            m = re.search(r"<([^>]+)>:$", line.strip())
            if m and not m.group(1).startswith("L"):
                on = kernel in m.group(1)
            continue
        if not on:
            continue
        text = line.split("//")[0].strip()
        m = re.search(r"//\s*([0-9A-Fa-f]+):", line)
        if not text or not m:
            continue
        t = re.search(r"<[^>]*\+0x([0-9a-fA-F]+)>", line)
        ins.append([text.split(None, 1)[0], text, int(t.group(1), 16) if t else None, int(m.group(1), 16)])
        addr_of.append(ins[-1][3])
    if not ins:
        return ins
    index = {a - addr_of[0]: i for i, a in enumerate(addr_of)}
    for i in ins:
        i[2] = index.get(i[2]) if i[2] is not None else None
    return ins


def is_branch(mn):
    return mn == "s_branch" or mn.startswith("s_cbranch")


def stretch(ins, a, b):
    """(instructions, taken branches) strictly between a and b on the shortest way from a to b."""
    best = {a: (0, 0)}
    heap = [(0, 0, a)]
    while heap:
        n, br, i = heapq.heappop(heap)
        if i == b:
            return n - 1, br
        if best.get(i, (n, br)) < (n, br) or i >= len(ins):
            continue
        mn, _, tgt = ins[i][:3]
        nxt = []
        if mn in ("s_endpgm", "s_barrier") and i != a:
            continue                                        # (no stretch crosses a barrier)
        if mn != "s_branch" and mn != "s_cbranch_execnz":
            nxt.append((i + 1, 0))
        if is_branch(mn) and mn != "s_cbranch_execz" and tgt is not None:
            nxt.append((tgt, 1))
        for j, taken in nxt:
            c = (n + 1, br + taken)
            if j not in best or c < best[j]:
                best[j] = c
                heapq.heappush(heap, (c[0], c[1], j))
    return None


def via(ins, a, mid, b):
    """stretch(a, b) through mid."""
    one, two = stretch(ins, a, mid), stretch(ins, mid, b)
    if one is None or two is None:
        return None
    return one[0] + two[0] + 1, one[1] + two[1]


def leader_loop(ins):
    """(first, last) of the iteration loop of the leader that does not record, workgroup scope: the
    smallest backward-branch range with two barriers and the head of a group sum whose only global
    stores are the granule's (sc0: workgroup scope) and the status word's (a dword)."""
    found = None
    for hi, (mn, _, lo, *_) in enumerate(ins):
        if not is_branch(mn) or lo is None or lo > hi:
            continue
        body = ins[lo:hi + 1]
        if sum(b[0] == "s_barrier" for b in body) != 2:
            continue
        if not any(b[0].startswith("v_xor_b32_dpp") and SUM_HEAD in b[1] for b in body):
            continue
        stores = [b[1].split() for b in body if b[0] == "global_store_dwordx2"]
        if not stores or any("sc0" not in s or "sc1" in s for s in stores):
            continue
        if found is None or hi - lo < found[1] - found[0]:
            found = (lo, hi)
    return found


def measure(ins):
    """{stretch: (instructions, taken branches)} of the leader's loop copy."""
    loop = leader_loop(ins)
    if loop is None:
        raise SystemExit("check_leader_stream: the leader's loop copy was not found")
    lo, hi = loop
    at = lambda pred, a=lo, b=hi: [i for i in range(a, b + 1) if pred(ins[i])]  # noqa: E731
    fmacs = at(lambda x: x[0].startswith("v_fmac_f64_dpp"))
    rsq = at(lambda x: x[0].startswith("v_rsq_f64"))[0]
    head = at(lambda x: x[0].startswith("v_xor_b32_dpp") and SUM_HEAD in x[1])[0]
    store = at(lambda x: x[0] == "global_store_dwordx2")[0]
    b2 = at(lambda x: x[0] == "s_barrier", fmacs[-1])[0]
    tags = at(lambda x: x[0].startswith("v_cmp_eq_u32_e32"), store, head)
    retire = at(lambda x: x[0] == "s_waitcnt" and "vmcnt" in x[1], head)[0]
    last_add = at(lambda x: x[0].startswith("v_add_f64"), head, retire)[-1]
    gam = at(lambda x: x[0] == "global_load_dwordx2" and "sc1" not in x[1].split(), fmacs[-1], b2)[-1]
    # (hipcc may rotate the loop so that the sigma2 step stands behind the back edge, at its top)
    floor = (at(lambda x: x[0].startswith("v_cmp_lt_f64"), retire) or
             at(lambda x: x[0].startswith("v_cmp_lt_f64"), lo, rsq))[0]
    b1 = [i for i in at(lambda x: x[0] == "s_barrier") if i != b2][0]
    out = {"draw -> B1": stretch(ins, rsq, b1), "pass -> B2": via(ins, fmacs[-1], gam, b2)}
    first = [i for i in fmacs if i > b1][0]
    u_read = at(lambda x: x[0].startswith("ds_read"), b1, first)
    if u_read:
        out["B1 -> u"] = stretch(ins, b1, u_read[0])
    out["B1 -> pass"] = stretch(ins, b1, first)
    out["B2 -> publish"] = stretch(ins, b2, store)
    for n, t in enumerate(tags):
        out[f"hit {n} -> sum"] = stretch(ins, t, head)
    out["sum -> draw"] = via(ins, last_add, floor, rsq)
    return out


def placement(ins):
    """Byte addresses of the two loop headers an iteration of the leader's copy branches back to:
    {"loop": the iteration loop's, "poll": the gather's poll loop's} (None where not found)."""
    loop = leader_loop(ins)
    if loop is None:
        return {"loop": None, "poll": None}
    lo, hi = loop
    poll = None
    for i in range(lo + 1, hi):
        mn, _, tgt = ins[i][:3]
        if not is_branch(mn) or tgt is None or not lo < tgt < i:
            continue
        body = ins[tgt:i + 1]
        if any(b[0] == "s_barrier" for b in body):
            continue
        if any(b[0] == "global_load_dwordx2" and "sc1" in b[1].split() for b in body):
            poll = ins[tgt][3]
            break
    return {"loop": ins[lo][3], "poll": poll}


def main(argv):
    sweep = "--no-placement" in argv        # (a placement sweep's build: print the addresses only)
    argv = [a for a in argv if a != "--no-placement"]
    if len(argv) != 1:
        print(__doc__, file=sys.stderr)
        return 2
    with tempfile.TemporaryDirectory() as tmp:
        ins = parse(device_asm(argv[0], tmp))
    got = measure(ins)
    # ("pass -> B2" first: the line's head is part of the gate's contract with its test)
    order = ["pass -> B2"] + [n for n in got if n != "pass -> B2"]
    print("check_leader_stream: " + "; ".join(
        f"{name} {got[name][0]} instructions {got[name][1]} taken" if got[name] else f"{name} not found"
        for name in order))
    where = placement(ins)
    print("check_leader_stream: placement " + "; ".join(
        f"{name} header at byte {a % 64} of its 64-byte line" if a is not None else f"{name} header not found"
        for name, a in where.items()))
    bad = []
    for name, limit in LIMITS.items():
        c = got.get(name)
        if c is None:
            bad.append(f"{name}: no such stretch in the leader's loop")
        elif c[0] > limit[0] or c[1] > limit[1]:
            bad.append(f"{name}: {c[0]} instructions, {c[1]} taken branches (limit {limit[0]}, {limit[1]})")
    extra = sorted(set(got) - set(LIMITS))
    bad += [f"{name}: a stretch without a limit" for name in extra]
    for name, want in ({} if sweep else PLACE).items():
        a = where.get(name)
        if a is None or a % PLACE_PERIOD != want:
            at = "not found" if a is None else f"at byte {a % PLACE_PERIOD}"
            bad.append(f"{name} header {at} of its {PLACE_PERIOD}-byte window, measured placement {want}: "
                       "adjust BMC_PLACE_PAD (kernels_gibbs.hip)")
    if bad:
        print("check_leader_stream: the leader's stream grew:", file=sys.stderr)
        for x in bad:
            print("  " + x, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
