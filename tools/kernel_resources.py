#!/usr/bin/env python3
"""Kernel resource table from a build log: one line per kernel (demangled name, SGPRs, VGPRs, AGPRs, scratch, spills, occupancy,
static LDS), sorted by name, from the remarks of a compile with -Rpass-analysis=kernel-resource-usage, e.g.

    make -C corenav_gp_amd/csrc CXXFLAGS="<the Makefile's> -Rpass-analysis=kernel-resource-usage" 2> build.log
    python tools/kernel_resources.py build.log [--only SUBSTRING ...] [--skip SUBSTRING ...] > profiles/<name>.txt

Two such tables of two trees are compared with diff: a kernel that did not move has an identical line."""
import re
import subprocess
import sys

KEYS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill", "Occupancy [waves/SIMD]",
        "LDS Size [bytes/block]")


def main(argv):
    only, skip, path = [], [], None
    it = iter(argv)
    for a in it:
        if a == "--only":
            only.append(next(it))
        elif a == "--skip":
            skip.append(next(it))
        else:
            path = a
    rows, cur = {}, None
    rx = re.compile(r"remark:\s+(.*?) \[-Rpass-analysis=kernel-resource-usage\]")
    for line in open(path, errors="replace"):
        m = rx.search(line)
        if not m:
            continue
        body = m.group(1).strip()
        if body.startswith("Function Name:"):
            cur = body.split(":", 1)[1].strip()
            rows[cur] = {}
        elif cur is not None and ":" in body:
            k, v = body.rsplit(":", 1)
            rows[cur][k.strip()] = v.strip()
    names = sorted(rows)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    out = []
    for mangled, name in zip(names, dem):
        if only and not any(s in name for s in only):
            continue
        if any(s in name for s in skip):
            continue
        out.append(name + "\t" + "\t".join("%s: %s" % (k, rows[mangled].get(k, "?")) for k in KEYS))
    print("\n".join(sorted(out)))


if __name__ == "__main__":
    main(sys.argv[1:])
