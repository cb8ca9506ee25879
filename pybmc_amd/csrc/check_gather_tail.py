#!/usr/bin/env python3
"""Build-time gate: the group sum behind a granule gather never waits for a poll.

``granule_gather1`` (bmc_loop.h) keeps DEPTH reads in flight; at the hit the later ones are still
travelling.  ``exchange_sum`` keeps their registers live across ``granule_sum1`` and retires them
behind its last add.  If hipcc instead gives a pending read's destination to a temporary of the
sum, it must put ``s_waitcnt vmcnt(0)`` in front of that temporary's first write -- in the middle
of the serial path, where the leader then stalls for the rest of a load round trip in every
iteration.  This script disassembles the gfx950 code objects of the given host objects and fails
the build when, in any kernel, an ``s_waitcnt`` that waits on ``vmcnt`` stands between a
``v_xor_b32_dpp ... quad_perm:[1,0,3,2]`` (the first instruction of ``granule_sum1``, which occurs
nowhere else) and the eighth ``v_readlane_b32`` after it (the last lane read of the sum).

The leader of the SMALLG kernels polls through one asm statement (``granule_gather1_asm``) whose
reads hipcc does not see: they land in the fixed registers POLL_REGS, one of them after the
statement has ended, and are retired by an explicit ``s_waitcnt vmcnt(0)`` behind the sum.  Second
rule: from a ``global_load_dwordx2`` into one of POLL_REGS up to the next wait for ``vmcnt(0)``, no
instruction but the statement's own polls may write a register of POLL_REGS -- a pending read would
land in a register that hipcc gave to something else.
Usage: check_gather_tail.py <file.o>...
"""
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_dpp_hazard import device_asm  # noqa: E402

# Kernels the gate does not hold: substring of the mangled name -> reason.  Empty, and no kernel
# needs it: every instantiation holds the trailing read across the sum without spilling.
EXEMPT = {}

READLANES = 8
# the registers the asm gather's reads land in (BMC_POLL_QA, BMC_POLL_QB in bmc_loop.h)
POLL_REGS = ((124, 125), (126, 127))
POLL_SET = {r for pair in POLL_REGS for r in pair}


def waits_on_vmcnt(text):
    """True when an s_waitcnt's operand names vmcnt (a raw immediate counts too: it sets all)."""
    ops = text.split(None, 1)[1] if len(text.split(None, 1)) > 1 else ""
    return "vmcnt" in ops or re.match(r"^\s*(0x[0-9a-f]+|\d+)\s*$", ops) is not None


def vgprs(operand):
    """The VGPR numbers an operand names: v7 -> {7}, v[4:5] -> {4, 5}, anything else -> {}."""
    m = re.match(r"^-?\|?v(\d+)\|?$", operand)
    if m:
        return {int(m.group(1))}
    m = re.match(r"^-?v\[(\d+):(\d+)\]$", operand)
    return set(range(int(m.group(1)), int(m.group(2)) + 1)) if m else set()


def written_vgprs(text):
    """The VGPRs an instruction writes: the first operand of a VALU instruction or of a load."""
    parts = text.split(None, 1)
    mn = parts[0]
    if len(parts) < 2 or "store" in mn or mn.startswith("ds_write"):
        return set()
    if not (mn.startswith("v_") or "load" in mn or mn.startswith("ds_read")):
        return set()
    return vgprs(parts[1].split(",")[0].strip())


def waits_for_all_vmem(text):
    """True for an s_waitcnt that leaves no load pending: vmcnt(0), or a raw immediate."""
    ops = text.split(None, 1)[1] if len(text.split(None, 1)) > 1 else ""
    return "vmcnt(0)" in ops or re.match(r"^\s*(0x[0-9a-f]+|\d+)\s*$", ops) is not None


def scan_polls(lines):
    """lines: disassembly text.  Returns (asm gathers checked, list of findings): writes to a
    register of POLL_REGS while a read of the asm gather may be pending.  The statement is known
    by its opening: a poll into the first pair of POLL_REGS and, behind nothing but s_nop, a poll
    into the second (hipcc's own gathers may use these registers too; they are its to count)."""
    func, pending, n, bad = "?", False, 0, []
    text_of = []
    for raw in lines:
        line = raw.rstrip("\n")
        if not line.startswith("\t") and not line.startswith(" "):
            m = re.search(r"<([^>]+)>:$", line.strip())
            text_of.append(("func", m.group(1)) if m and not m.group(1).startswith("L") else ("", ""))
            continue
        text_of.append(("ins", line.split("//")[0].strip()))

    def poll_into(text, pair):
        return (text.split(None, 1)[0] == "global_load_dwordx2" and "sc1" in text.split()
                and tuple(sorted(written_vgprs(text))) == pair)

    for i, (kind, text) in enumerate(text_of):
        if kind == "func":
            func, pending = text, False
        if kind != "ins" or not text:
            continue
        mn = text.split(None, 1)[0]
        if not pending and poll_into(text, POLL_REGS[0]):
            nxt = [t for k, t in text_of[i + 1:i + 12] if k == "ins" and t and not t.startswith("s_nop")]
            if nxt and poll_into(nxt[0], POLL_REGS[1]):
                pending = True
                n += 1
        elif not pending:
            continue
        elif poll_into(text, POLL_REGS[0]) or poll_into(text, POLL_REGS[1]):
            continue                   # (the statement's own reads)
        elif (mn == "s_waitcnt" and waits_for_all_vmem(text)) or mn == "s_endpgm":
            pending = False
        elif written_vgprs(text) & POLL_SET:
            bad.append(f"{func}: {text}  writes a register of a pending poll")
    return n, bad


def scan(lines):
    """lines: disassembly text.  Returns (sums checked, sums exempted, list of findings)."""
    func = "?"
    left = 0            # v_readlane_b32 still to come in the open window (0: no window)
    n_sum, n_exempt, bad = 0, 0, []
    held = True         # the open window belongs to a kernel the gate holds (not in EXEMPT)
    for raw in lines:
        line = raw.rstrip("\n")
        if not line.startswith("\t") and not line.startswith(" "):
            m = re.search(r"<([^>]+)>:$", line.strip())
            if m and not m.group(1).startswith("L"):
                func = m.group(1)
                left = 0
            continue
        text = line.split("//")[0].strip()
        if not text:
            continue
        mn = text.split(None, 1)[0]
        if mn.startswith("v_xor_b32_dpp") and "quad_perm:[1,0,3,2]" in text:
            if left == READLANES:      # the xor swap's second half: the same sum
                continue
            held = not any(k in func for k in EXEMPT)
            n_sum += held
            n_exempt += not held
            left = READLANES
            continue
        if left == 0:
            continue
        if mn.startswith("v_readlane_b32"):
            left -= 1
        elif held and mn == "s_waitcnt" and waits_on_vmcnt(text):
            bad.append(f"{func}: {text}  inside the group sum ({READLANES - left} of {READLANES} "
                       f"lane reads done)")
        elif mn == "s_endpgm":
            left = 0
    return n_sum, n_exempt, bad


def main(argv):
    total, exempt, polls, bad, bad_polls = 0, 0, 0, [], []
    with tempfile.TemporaryDirectory() as tmp:
        for obj in argv:
            lines = list(device_asm(obj, tmp))
            n, e, b = scan(lines)
            total += n
            exempt += e
            bad += [f"{os.path.basename(obj)}: {x}" for x in b]
            n, b = scan_polls(lines)
            polls += n
            bad_polls += [f"{os.path.basename(obj)}: {x}" for x in b]
    if bad:
        print(f"check_gather_tail: {len(bad)} wait(s) on vmcnt inside a group sum:", file=sys.stderr)
        for x in bad[:40]:
            print("  " + x, file=sys.stderr)
    if bad_polls:
        print(f"check_gather_tail: {len(bad_polls)} write(s) to a register of a pending poll:", file=sys.stderr)
        for x in bad_polls[:40]:
            print("  " + x, file=sys.stderr)
    if bad or bad_polls:
        return 1
    print(f"check_gather_tail: {total} group sums checked ({exempt} exempt), none waits on vmcnt; "
          f"{polls} asm gathers checked, none has a pending poll's register written")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
