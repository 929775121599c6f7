#!/usr/bin/env python3
"""Compare the gfx950 instruction streams of two builds, symbol by symbol.

The gate of a refactor that must leave the device code as it is: every kernel
present in both builds has the same instructions (mnemonics, operands,
encodings, addresses relative to the symbol); symbols may only disappear.

    tools/dump_isa.sh <parent>/build/sha1_kernels.o parent_sha1_kernels.s   (and the new build's)
    tools/isa_compare.py --parent-commit b770692 --new-commit <id> --out profiles/NAME.json \\
        sha1_kernels.o=parent_sha1_kernels.s:new_sha1_kernels.s  [more objects ...]

Exit status 1 if a symbol present in both differs or a symbol appeared.
"""
import argparse
import hashlib
import json
import re
import subprocess
import sys

SYM = re.compile(r"^([0-9a-f]{16}) <(.+)>:$")
INS = re.compile(r"^\t(.*?)\s*// ([0-9A-F]{12}): (.*)$")


def symbols(path):
    """symbol -> list of 'offset: encoding [<target>] text' lines."""
    out, cur, base = {}, None, 0
    for line in open(path):
        line = line.rstrip("\n")
        m = SYM.match(line)
        if m:
            base, cur = int(m.group(1), 16), out.setdefault(m.group(2), [])
            continue
        m = INS.match(line)
        if m and cur is not None:
            cur.append("%x: %s %s" % (int(m.group(2), 16) - base, m.group(3), m.group(1)))
    return out


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-commit", required=True)
    ap.add_argument("--new-commit", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--note", action="append", default=[], help="free text kept in the record")
    ap.add_argument("objects", nargs="+", help="NAME=parent.s:new.s")
    a = ap.parse_args()
    hipcc = subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True).stdout.splitlines()
    rec = {"parent": a.parent_commit, "new": a.new_commit, "hipcc": [l for l in hipcc if "version" in l],
           "notes": a.note, "objects": {}}
    bad = 0
    for spec in a.objects:
        name, files = spec.split("=")
        old, new = (symbols(f) for f in files.split(":"))
        rows = {}
        for s in sorted(set(old) | set(new)):
            o, n = old.get(s), new.get(s)
            state = "removed" if n is None else "added" if o is None else "same" if o == n else "differs"
            bad += state in ("added", "differs")
            rows[s] = {"parent_instructions": o and len(o), "new_instructions": n and len(n),
                       "parent_hash": o and digest(o), "new_hash": n and digest(n), "state": state}
        rec["objects"][name] = rows
        count = {k: sum(r["state"] == k for r in rows.values()) for k in ("same", "removed", "added", "differs")}
        print(name, count)
        for s, r in rows.items():
            if r["state"] in ("added", "differs"):
                print("  %s: %s" % (r["state"], s))
    json.dump(rec, open(a.out, "w"), indent=1)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
