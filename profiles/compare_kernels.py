#!/usr/bin/env python3
"""Compares two builds of the HIP kernels by mangled kernel name, on the CPU.

    python profiles/compare_kernels.py old_dir new_dir [--all]

Both directories hold the assembly of the same .hip files, one NAME.s each, made with build.py's FLAGS:

    hipcc <FLAGS> --cuda-device-only -S csrc/NAME.hip -o DIR/NAME.s

One row per kernel: whether every .amdhsa_* directive (VGPR / AGPR / SGPR counts, LDS, scratch, the occupancy inputs) is
the same, the instruction count in both builds and the MFMA count in both builds.  Rows of kernels whose text is identical
are printed only with --all.  Exit status 1 if a kernel exists in one build only, a directive differs or an MFMA count
differs: a refactor that is meant to leave the kernels alone must not move any of these.  A different instruction count is
reported, not failed: the scheduler reorders independent instructions when the source is merely regrouped.
"""
import os
import re
import sys

_LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")
_KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
_INSN = re.compile(r"^\s+([a-z][a-z0-9_]*)\b")


def kernels(path):
    """{name: (directives, instruction lines)} of one assembly file."""
    bodies, cur = {}, None          # label -> instruction lines up to the end of its function
    directives, desc = {}, None     # kernel -> {directive: value}
    for line in open(path):
        line = line.split(";")[0].rstrip()
        m = _KERNEL.match(line)
        if m:
            desc = directives.setdefault(m.group(1), {})
        elif desc is not None:
            if ".end_amdhsa_kernel" in line:
                desc = None
            elif line.strip().startswith(".amdhsa_"):
                key, _, val = line.strip().partition(" ")
                desc[key] = val.strip()
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif _LABEL.match(line) and not line.startswith(".L"):
            cur = bodies.setdefault(_LABEL.match(line).group(1), [])
        elif cur is not None and _INSN.match(line):
            cur.append(" ".join(line.split()))
    return {k: (d, bodies.get(k, [])) for k, d in directives.items()}


def main(argv):
    show_all = "--all" in argv
    old_dir, new_dir = [a for a in argv if not a.startswith("--")]
    bad = same_text = total = 0
    for f in sorted(set(os.listdir(old_dir)) | set(os.listdir(new_dir))):
        if not f.endswith(".s"):
            continue
        paths = [os.path.join(d, f) for d in (old_dir, new_dir)]
        if not all(os.path.exists(p) for p in paths):
            print(f"{f}: present in one build only")
            bad += 1
            continue
        old, new = kernels(paths[0]), kernels(paths[1])
        for name in sorted(set(old) | set(new)):
            total += 1
            if name not in old or name not in new:
                print(f"{f} {name}: MISSING in the {'old' if name not in old else 'new'} build")
                bad += 1
                continue
            (d0, i0), (d1, i1) = old[name], new[name]
            diff = sorted(k for k in set(d0) | set(d1) if d0.get(k) != d1.get(k))
            m0, m1 = (sum(x.startswith("v_mfma") for x in i) for i in (i0, i1))
            if i0 == i1 and not diff:
                same_text += 1
                if not show_all:
                    continue
            ok = not diff and m0 == m1
            bad += not ok
            hist = "same opcodes" if sorted(x.split()[0] for x in i0) == sorted(x.split()[0] for x in i1) else "opcodes differ"
            print(f"{f} {name}: directives {'equal' if not diff else 'DIFFER ' + ','.join(diff)}; "
                  f"instructions {len(i0)} -> {len(i1)} ({len(i1) - len(i0):+d}, {hist}); mfma {m0} -> {m1}")
    print(f"{total} kernels, {same_text} text-identical, {bad} failed")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
