"""Per-kernel VGPR / SGPR / spill / LDS / occupancy of the gfx950 build of one or
more HIP sources, from the compiler's kernel-resource-usage remarks, optionally
diffed against the same sources of another tree.  A source named *_p16.hip gets
the scheduler flag the Makefile gives the P = 16 translation unit, so one call
lists the whole library; any source may carry flags of its own after an '@'
(for a tree that compiles one file twice: 'k.hip' and 'k.hip@-DSECOND_UNIT -mllvm -amdgpu-use-amdgpu-trackers=1'):

  python scripts/kernel_resources.py simd-ray-tracer_amd/csrc/*.hip
  python scripts/kernel_resources.py simd-ray-tracer_amd/csrc/*.hip --diff-tree ../other/checkout
  python scripts/kernel_resources.py simd-ray-tracer_amd/csrc/rt_trace.hip --filter Li4E --flags "-DRTK_STATS"

usage: kernel_resources.py <src.hip>... [--filter text] [--flags "-DX=1"] [--diff-tree dir | --diff other.hip...]
(--diff-tree: the same paths under another checkout's root; --diff: explicit sources, any number)
"""
import argparse
import os
import re
import subprocess

HIPCC = "/opt/rocm/bin/hipcc"
P16_FLAGS = ["-mllvm", "-amdgpu-use-amdgpu-trackers=1"]  # simd-ray-tracer_amd/Makefile P16FLAGS


def base_flags(src):
    csrc = os.path.dirname(os.path.abspath(src))
    return ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC",
            "-I" + os.path.join(csrc, "..", "..", "include"), "-I" + csrc, "-fno-slp-vectorize",
            "--offload-device-only", "-c", "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"]


def resources(sources, flags):
    out = {}
    procs = []
    for spec in sources:
        s, _, own = spec.partition("@")
        procs.append(subprocess.Popen([HIPCC, *base_flags(s), *(P16_FLAGS if s.endswith("_p16.hip") else []),
                                       *own.split(), *flags, s], stderr=subprocess.PIPE, text=True))
    for p in procs:
        cur = None
        for line in p.communicate()[1].splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                cur = m.group(1)
                out[cur] = {}
                continue
            m = re.search(r"remark: .*?(VGPRs|SGPRs|VGPRs Spill|SGPRs Spill|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\d+)",
                          line)
            if m and cur:
                out[cur][m.group(1)] = int(m.group(2))
    return out


def fmt(v):
    return (f"v{v.get('VGPRs', -1):4d} s{v.get('SGPRs', -1):4d} vsp{v.get('VGPRs Spill', -1):3d} "
            f"ssp{v.get('SGPRs Spill', -1):3d} lds{v.get('LDS Size [bytes/block]', -1):6d} "
            f"occ{v.get('Occupancy [waves/SIMD]', -1):2d}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("sources", nargs="+")
    ap.add_argument("--filter", default="", help="list only kernels whose symbol contains this")
    ap.add_argument("--flags", default="", help="extra compiler flags for every source")
    ap.add_argument("--diff", nargs="+", default=None, help="sources to diff against")
    ap.add_argument("--diff-tree", default=None, help="another checkout's root: the same relative paths")
    args = ap.parse_args()
    flags = args.flags.split()
    other = args.diff or ([os.path.join(args.diff_tree, s) for s in args.sources] if args.diff_tree else None)
    r = resources(args.sources, flags)
    o = resources(other, flags) if other else {}
    for name in sorted(r):
        if args.filter not in name:
            continue
        line = f"{name[:88]:88s} {fmt(r[name])}"
        if other:
            if name not in o:
                line += "   (new)"
            elif o[name] != r[name]:
                line += f"   was {fmt(o[name])}"
            else:
                continue
        print(line)
    if other:
        gone = sorted(set(o) - set(r))
        for name in gone:
            print(f"{name[:88]:88s} (gone)")
        changed = sum(1 for k in r if k in o and o[k] != r[k])
        print(f"{len(r)} kernels, {len(o)} on the other side: {changed} changed, "
              f"{len(set(r) - set(o))} new, {len(gone)} gone")


if __name__ == "__main__":
    main()
