#!/usr/bin/env python3
"""isa_same.py PARENT.s BRANCH.s -- are the kernels of two device assemblies the same text?

Both files come from `hipcc <the Makefile's flags> --cuda-device-only -S x.hip`.
For every kernel of PARENT.s (every `.amdhsa_kernel` descriptor) the text from
its label to its `.Lfunc_end` and its descriptor are compared with BRANCH.s,
after dropping assembler comments (from `;`) and the function number in local
labels (`.LBB<n>_`, `.Lfunc_end<n>`), which moves when a kernel before it is
removed.  Prints `same`, `DIFF` or `removed` per kernel (`added` for one only in
BRANCH.s) and exits non-zero on any DIFF.  Text only: a refactor that must not
change the product is proven by identical assembly, whatever the instructions.
"""
import re
import sys


def kernels(path):
    lines = open(path).read().split("\n")
    out = {}
    for i, line in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if not m:
            continue
        name = m.group(1)
        end = next(j for j in range(i, len(lines)) if ".end_amdhsa_kernel" in lines[j])
        start = next(j for j in range(len(lines)) if lines[j].startswith(name + ":"))
        fend = next(j for j in range(start, len(lines)) if lines[j].startswith(".Lfunc_end"))
        text = []
        for raw in lines[start:fend + 1] + lines[i:end + 1]:
            t = raw.split(";", 1)[0].rstrip()
            t = re.sub(r"\.LBB\d+_", ".LBB_", t)
            t = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", t)
            if t.strip():
                text.append(t)
        out[name] = text
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    parent, branch = kernels(sys.argv[1]), kernels(sys.argv[2])
    print("%s -> %s" % (sys.argv[1], sys.argv[2]))
    diffs = 0
    for name in sorted(set(parent) | set(branch)):
        if name not in branch:
            verdict = "removed"
        elif name not in parent:
            verdict = "added"
        else:
            verdict = "same" if parent[name] == branch[name] else "DIFF"
        diffs += verdict == "DIFF"
        print("  %-7s %s (%d lines)" % (verdict, name, len(parent.get(name) or branch[name])))
    print("  %d kernels, %d DIFF" % (len(set(parent) | set(branch)), diffs))
    sys.exit(1 if diffs else 0)


if __name__ == "__main__":
    main()
