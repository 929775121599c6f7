#!/usr/bin/env python3
"""Address parity of a kernel's `v_add_u32_dpp` instructions, from a
disassembly written by tools/dump_isa.sh.  A DPP add that starts at an address
4 mod 8 costs ~5 cycles more than one at an 8-byte boundary (DESIGN.md
section 5, fact 5), and hipcc does not say when a 4-byte instruction of its
own (an s_waitcnt, a hazard s_nop, a v_xor) has shifted the quad consumer's
rounds.  Run this after any change to the consumer:

    tools/dump_isa.sh congestion-control-with-bittorren_amd/build/sha1_kernels.o /tmp/k.s
    tools/dpp_parity.py /tmp/k.s [kernel symbol]

Prints the DPP adds as runs of [address mod 8, count] in program order, and
exits 1 if any of them is misaligned.  Default kernel: the quad split shape.
"""
import re
import sys

QUAD = "_Z17sha1_split_kernelILi4ELi1ELi41029ELi2EEv9BatchArgs"


def main():
    path = sys.argv[1]
    sym = sys.argv[2] if len(sys.argv) > 2 else QUAD
    cur, runs, total = None, [], 0
    for line in open(path):
        m = re.match(r"^[0-9a-f]+ <(\w+)>:", line)
        if m:
            cur = m.group(1)
            continue
        if cur != sym:
            continue
        m = re.match(r"^\s+v_add_u32_dpp\b.*//\s*([0-9A-Fa-f]+):", line)
        if not m:
            continue
        total += 1
        par = int(m.group(1), 16) % 8
        if runs and runs[-1][0] == par:
            runs[-1][1] += 1
        else:
            runs.append([par, 1])
    bad = sum(n for par, n in runs if par)
    print(f"{sym}: {total} v_add_u32_dpp, {bad} misaligned; runs [address mod 8, count]: {runs}")
    if total == 0:
        sys.exit(f"no v_add_u32_dpp found in {sym}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
