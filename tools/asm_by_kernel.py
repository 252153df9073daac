#!/usr/bin/env python3
"""Compare two builds of the device code kernel by kernel: did a change of the sources change what any kernel compiles to?

    hipcc --offload-arch=gfx950 <flags of pgdrive_amd/build.py> --cuda-device-only -S -o before.s pgdrive_amd/csrc/pgd_engine.hip
    ... the same at the other commit -> after.s
    tools/asm_by_kernel.py before.s after.s        (or two directories: the *.s files of the same name are compared pair by pair)

Per kernel symbol of the FIRST build, two texts are compared: the instructions between the symbol's label and its .Lfunc_end (comments,
.loc / .file lines dropped, local labels renumbered in order of appearance) and the symbol's .amdhsa_kernel ... .end_amdhsa_kernel
block (registers, LDS, scratch).  One line per symbol that differs or is missing from the second build; exit status 1 if there is one.
No GPU needed."""
import os
import re
import sys

LOCAL = re.compile(r"\.L[A-Za-z_$]*\d+(?:_\d+)?")


def clean(line):
    line = line.split(";", 1)[0].strip()
    return "" if line.startswith((".loc", ".file")) else line


def renumber(lines):
    names = {}
    return [LOCAL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), x) for x in lines]


def kernels(path):
    """{symbol: (instruction text, kernel descriptor block)} of one assembly file."""
    with open(path) as f:
        lines = [c for c in map(clean, f) if c]
    desc, start = {}, {}
    for k, line in enumerate(lines):
        if line.startswith(".amdhsa_kernel "):
            end = lines.index(".end_amdhsa_kernel", k)
            desc[line.split()[1]] = lines[k:end + 1]
        elif line.endswith(":") and not line.startswith(".L"):
            start[line[:-1]] = k
    out = {}
    for sym, d in desc.items():
        k = start[sym] + 1
        end = next(j for j in range(k, len(lines)) if lines[j].startswith(".Lfunc_end"))
        out[sym] = (renumber(lines[k:end]), d)
    return out


def compare(a_path, b_path):
    a, b = kernels(a_path), kernels(b_path)
    differing = 0
    for sym in sorted(a):
        if sym not in b:
            what = "missing from the second build"
        elif a[sym][0] != b[sym][0]:
            first = next((k for k, (x, y) in enumerate(zip(a[sym][0], b[sym][0])) if x != y), min(len(a[sym][0]), len(b[sym][0])))
            what = "instructions differ: %d -> %d lines, first at line %d" % (len(a[sym][0]), len(b[sym][0]), first)
        elif a[sym][1] != b[sym][1]:
            what = "kernel descriptor differs: " + ", ".join(x for x in a[sym][1] if x not in b[sym][1])
        else:
            continue
        differing += 1
        print("%s: %s: %s" % (os.path.basename(a_path), sym, what))
    print("%s: %d kernels compared / %d differing" % (os.path.basename(a_path), len(a), differing))
    return differing


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    a, b = argv[1:]
    if os.path.isdir(a):
        pairs = [(os.path.join(a, n), os.path.join(b, n)) for n in sorted(os.listdir(a)) if n.endswith(".s")]
    else:
        pairs = [(a, b)]
    return 1 if sum(compare(x, y) for x, y in pairs) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
