#!/usr/bin/env python
"""Compare two gfx950 device-assembly files (hipcc ... --cuda-device-only -S) kernel by kernel.

    python tools/asm_same.py PARENT.s NEW.s [--allow REGEX]

A kernel added to the translation unit renumbers the functions after it, and the number appears in
every local label of those functions (.LBB<function>_<block>, also in the loop comments), so a plain
diff of the two files shows every later kernel as changed.  This compares each function's text with that
number and the comment padding removed and the __hip_cuid symbol masked; nothing else is normalised.
Prints the kernels only one side has and those whose code differs; exits 1 if a differing kernel does
not match --allow."""
import argparse
import re
import sys


def kernels(path):
    txt = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", open(path).read())
    out = {}
    for m in re.finditer(r"^\s*\.type\s+(\S+),@function\n(.*?)^\.Lfunc_end\d+:", txt, flags=re.S | re.M):
        body = re.sub(r"(BB|JTI|CPI)\d+_", r"\1_", m.group(2))
        out[m.group(1)] = re.sub(r"[ \t]+;", " ;", body)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--allow", default=None, help="regex of kernel symbols that may differ")
    args = ap.parse_args()
    a, b = kernels(args.parent), kernels(args.new)
    differing = [k for k in a if k in b and a[k] != b[k]]
    print(f"{len(a)} kernels in {args.parent}, {len(b)} in {args.new}; "
          f"{len(set(b) - set(a))} added, {len(set(a) - set(b))} removed, {len(differing)} differing")
    for k in sorted(set(a) - set(b)):
        print("  removed  ", k)
    for k in sorted(set(b) - set(a)):
        print("  added    ", k)
    bad = 0
    for k in differing:
        ok = args.allow is not None and re.search(args.allow, k) is not None
        bad += not ok
        print("  differing", k, "(allowed)" if ok else "")
    sys.exit(1 if bad or set(a) - set(b) else 0)


if __name__ == "__main__":
    main()
