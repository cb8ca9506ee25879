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


def waits_on_vmcnt(text):
    """True when an s_waitcnt's operand names vmcnt (a raw immediate counts too: it sets all)."""
    ops = text.split(None, 1)[1] if len(text.split(None, 1)) > 1 else ""
    return "vmcnt" in ops or re.match(r"^\s*(0x[0-9a-f]+|\d+)\s*$", ops) is not None


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
    total, exempt, bad = 0, 0, []
    with tempfile.TemporaryDirectory() as tmp:
        for obj in argv:
            n, e, b = scan(device_asm(obj, tmp))
            total += n
            exempt += e
            bad += [f"{os.path.basename(obj)}: {x}" for x in b]
    if bad:
        print(f"check_gather_tail: {len(bad)} wait(s) on vmcnt inside a group sum:", file=sys.stderr)
        for x in bad[:40]:
            print("  " + x, file=sys.stderr)
        return 1
    print(f"check_gather_tail: {total} group sums checked ({exempt} exempt), none waits on vmcnt")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
