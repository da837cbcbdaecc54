#!/usr/bin/env python3
"""Which kernels differ between two device-only -S outputs of b9_kernels.hip, and by how many instructions.

    hipcc <base_amd/build.py's HIP_FLAGS> --cuda-device-only -S -o old.s -x hip base_amd/csrc/b9_kernels.hip     (on each tree;
    python tools/isa_diff.py old.s new.s [filter-substring]                              tools/kernel_resources.py leaves one in /tmp)

Each file is split at the kernel labels (a `_Z...:` line up to its `.Lfunc_end`); comments, directives and blank lines are
dropped and local labels renumbered in order of appearance, so that two kernels compare equal exactly when their instruction
streams do.  Prints one line per kernel that differs or exists on one side only, then the totals.  It compares text only."""
import re
import subprocess
import sys


def kernels(path):
    out, name, body, labels = {}, None, [], {}
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body, labels = m.group(1), [], {}
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = [re.sub(r"\.LBB\d+_\d+", lambda k: labels.setdefault(k.group(0), f"L{len(labels)}"), s) for s in body]
            name = None
            continue
        s = line.split(";", 1)[0].strip()
        if not s or (s.startswith(".") and not s.startswith(".LBB")):
            continue
        body.append(re.sub(r"\s+", " ", s))
    return out


def main():
    if len(sys.argv) not in (3, 4):
        raise SystemExit(__doc__)
    old, new, flt = kernels(sys.argv[1]), kernels(sys.argv[2]), sys.argv[3] if len(sys.argv) == 4 else ""
    names = sorted(set(old) | set(new))
    dem = dict(zip(names, subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.splitlines()))
    short = {n: re.sub(r"\(.*", "", dem.get(n, n)).replace("void ", "") for n in names}
    same = 0
    for n in names:
        if flt and flt not in short[n]:
            continue
        count = lambda body: sum(1 for s in body if not s.endswith(":"))
        if n not in old:
            print(f"only in new   {short[n]:60s} {count(new[n]):6d}")
        elif n not in new:
            print(f"only in old   {short[n]:60s} {count(old[n]):6d}")
        elif old[n] != new[n]:
            print(f"differs       {short[n]:60s} {count(old[n]):6d} -> {count(new[n]):6d}  ({count(new[n]) - count(old[n]):+d})")
        else:
            same += 1
    print(f"{same} kernels identical, {len(old)} in old, {len(new)} in new")


if __name__ == "__main__":
    main()
