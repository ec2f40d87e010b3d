"""Kernel-by-kernel comparison of two sets of gfx950 assembly listings (hipcc
--cuda-device-only -S), for checking that a source refactor left the machine
code alone: the kernel symbols of both sides, each kernel's instruction
sequence and its kernel descriptor (.amdhsa_* block: registers, spills'
scratch, LDS).  Local labels carry their function's index in its translation
unit (.LBB12_3), which changes when kernels move between files, so that index
is dropped; comments are dropped.

usage: python scripts/isa_diff.py --a old1.s [old2.s ...] --b new1.s [new2.s ...]
exit status 1 when the symbol sets differ or any kernel differs.
"""
import re
import sys

LABEL = re.compile(r"\.L(BB|func_end|func_begin|tmp|JTI)(\d+)(_\d+)?")


def norm(line):
    line = line.split(";", 1)[0].rstrip()
    return LABEL.sub(lambda m: f".L{m.group(1)}{m.group(3) or ''}", line)


def kernels(paths):
    """{kernel symbol: (instruction lines, descriptor lines)} over the listings."""
    body, desc = {}, {}
    for path in paths:
        cur = dsc = None
        for raw in open(path):
            line = norm(raw)
            if not line.strip():
                continue
            m = re.match(r"(\w+):$", line)
            if m and not line.startswith(".L"):
                cur = m.group(1)
                body[cur] = []
                continue
            if line.lstrip().startswith(".amdhsa_kernel "):
                dsc = line.split()[1]
                desc[dsc] = []
                continue
            if line.lstrip().startswith(".end_amdhsa_kernel"):
                dsc = None
                continue
            if dsc is not None:
                desc[dsc].append(line.strip())
            elif cur is not None:
                if re.match(r"\s*\.Lfunc_end", line):
                    cur = None
                else:
                    body[cur].append(line.strip())
    return {k: (body.get(k, []), desc[k]) for k in desc}


def main():
    argv = sys.argv[1:]
    a = kernels(argv[argv.index("--a") + 1:argv.index("--b")])
    b = kernels(argv[argv.index("--b") + 1:])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    for k in only_a:
        print(f"only in a: {k}")
    for k in only_b:
        print(f"only in b: {k}")
    differ = 0
    for k in sorted(set(a) & set(b)):
        if a[k] != b[k]:
            differ += 1
            what = "instructions" if a[k][0] != b[k][0] else "descriptor"
            print(f"differs ({what}; {len(a[k][0])} against {len(b[k][0])} lines): {k}")
    common = len(set(a) & set(b))
    insns = sum(len(v[0]) for v in b.values())
    print(f"kernels: a {len(a)}, b {len(b)}, compared {common}, identical {common - differ}, differing {differ}; "
          f"{insns} instruction and label lines in b")
    sys.exit(1 if only_a or only_b or differ else 0)


if __name__ == "__main__":
    main()
