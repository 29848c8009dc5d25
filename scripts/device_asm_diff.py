#!/usr/bin/env python3
"""Are two builds of one ``.hip`` file the same device code? For a host-side refactor.

    hipcc <the flags of ops/_lib.build()> --cuda-device-only -S old.hip -o old.s   (and new.s)
    python scripts/device_asm_diff.py old.s new.s

Compares every function between its label and ``.Lfunc_end`` instruction line by instruction
line (comment lines and trailing ``;`` comments stripped; the function's index inside block labels
dropped, since functions may come out in another order), and each kernel's ``.amdhsa_`` resource
lines. Prints the functions that differ and ``N of M differ``; exit status 1 if N > 0."""
import re
import sys


def functions(path):
    """{function: its instruction lines}, {kernel: its .amdhsa_ lines} of one assembly file."""
    text = open(path).read()
    names = set(re.findall(r"\.type\s+(\w+),@function", text))
    fns, res, name, desc = {}, {}, None, None
    for raw in text.splitlines():
        # block labels carry the function's position in the file (.LBB<function>_<block>), which
        # follows the order in which host code first names the kernels: keep the block number only
        line = re.sub(r"\.(LBB|LJTI)\d+_", r".\1_", raw.split(";")[0].strip())
        if not line:
            continue
        if name is None and line.endswith(":") and line[:-1] in names:
            name = line[:-1]
            fns[name] = []
        elif name is not None and line.startswith(".Lfunc_end"):
            name = None
        elif name is not None:
            fns[name].append(line)
        if line.startswith(".amdhsa_kernel "):
            desc = line.split()[1]
            res[desc] = []
        elif line.startswith(".end_amdhsa_kernel"):
            desc = None
        elif desc is not None:
            res[desc].append(line)
    return fns, res


def main(old, new):
    (f0, r0), (f1, r1) = functions(old), functions(new)
    every = sorted(set(f0) | set(f1))
    bad = [n for n in every if f0.get(n) != f1.get(n) or r0.get(n) != r1.get(n)]
    for n in bad:
        print("differs:", n)
    print(f"{len(bad)} of {len(every)} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
