#!/usr/bin/env python3
"""isa_diff.py [--allow-added] OLD_DIR NEW_DIR -- did a change leave the kernels as they were?

Each directory holds the device assembly of the kernel units, one .s per .hip file, compiled before and after the change with the
Makefile's HIPFLAGS:   hipcc $HIPFLAGS --cuda-device-only -S csrc/kernels_X.hip -o DIR/kernels_X.s
Kernels are paired by symbol.  Compared per kernel: its function body (from its label to its .Lfunc_end) and its
.amdhsa_kernel ... .end_amdhsa_kernel block, comments dropped and the per-file function number taken out of local labels (.LBB7_2 -> .LBB_2),
so that only a kernel's place in its file may change.  Prints the symbols added, removed and changed with the file each one's code came
from; exit status 1 on any difference (or a symbol defined twice in one directory), 0 if every kernel is identical.
--allow-added: a change that adds kernels -- ADDED lines are still printed but do not fail; REMOVED, DIFFERS, MOVED and TWICE do.
"""
import pathlib
import re
import sys

LOCAL = re.compile(r"\.L([A-Za-z_]+?)\d+(_\d+)?\b")


def kernels(directory):
    """symbol -> (file name, body lines, descriptor lines)"""
    out, twice = {}, []
    for path in sorted(pathlib.Path(directory).glob("*.s")):
        lines = [LOCAL.sub(r".L\1\2", l.split(";")[0].strip()) for l in path.read_text().splitlines()]
        lines = [l for l in lines if l]
        start = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":") and not l.startswith(".")}
        for i, l in enumerate(lines):
            if not l.startswith(".amdhsa_kernel "):
                continue
            sym = l.split()[1]
            body = lines[start[sym]:lines.index(".Lfunc_end:", start[sym])]
            desc = lines[i:lines.index(".end_amdhsa_kernel", i)]
            if sym in out:
                twice.append((sym, out[sym][0], path.name))
            out[sym] = (path.name, body, desc)
    return out, twice


def main():
    args = [a for a in sys.argv[1:] if a != "--allow-added"]
    allow_added = len(args) != len(sys.argv) - 1
    if len(args) != 2:
        sys.exit(__doc__)
    (old, old_twice), (new, new_twice) = kernels(args[0]), kernels(args[1])
    bad = added = 0
    for sym, a, b in old_twice + new_twice:
        print(f"TWICE    {sym}  ({a}, {b})"); bad += 1
    for sym in sorted(old.keys() - new.keys()):
        print(f"REMOVED  {sym}  (was in {old[sym][0]})"); bad += 1
    for sym in sorted(new.keys() - old.keys()):
        print(f"ADDED    {sym}  (in {new[sym][0]})"); added += 1
    if not allow_added:
        bad += added
    for sym in sorted(old.keys() & new.keys()):
        what = [n for n, k in (("body", 1), ("descriptor", 2)) if old[sym][k] != new[sym][k]]
        if what:
            print(f"DIFFERS  {sym}  ({' and '.join(what)}; {old[sym][0]} -> {new[sym][0]})"); bad += 1
        elif old[sym][0] != new[sym][0]:
            print(f"MOVED    {sym}  ({old[sym][0]} -> {new[sym][0]})"); bad += 1
    files = sorted({v[0] for v in new.values()})
    print(f"{len(old)} kernels before, {len(new)} after; per file after: " + ", ".join(f"{f} {sum(v[0] == f for v in new.values())}" for f in files))
    print(("IDENTICAL" if not added else f"EXISTING KERNELS IDENTICAL, {added} ADDED") if not bad else f"{bad} DIFFERENCES")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
