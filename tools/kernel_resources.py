#!/usr/bin/env python3
"""Per-kernel resources from device assembly (hipcc --cuda-device-only -S): one line per kernel symbol with VGPRs, AGPRs, SGPRs,
scratch and LDS bytes, and the waves per SIMD that the vector registers allow (512 / (.vgpr_count rounded up to 8), at most 8; .vgpr_count is
the combined count - the architected VGPRs plus the AGPRs listed beside it).
  tools/kernel_resources.py a.s b.s ... > profiles/rNN_kernel_resources.txt"""
import os
import re
import subprocess
import sys

KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(path):
    cur = {}
    for line in open(path):
        m = re.match(r"\s*-?\s*\.(\w+):\s*(\S+)\s*$", line)
        if not m:
            continue
        k, v = m.groups()
        if k in KEYS:
            cur[k] = int(v)
        elif k == "name" and v.startswith("_Z") and "group_segment_fixed_size" in cur:   # the kernel's own .name follows its sizes
            cur["name"] = v
        if k == "wavefront_size" and "name" in cur:                                       # last key of a kernel's record
            yield cur
            cur = {}


def main(paths):
    rows = []
    for p in paths:
        for k in kernels(p):
            regs = (k["vgpr_count"] + 7) // 8 * 8      # .vgpr_count is the combined count: it includes the AGPRs on gfx950
            rows.append((os.path.basename(p)[:-2], k, min(8, 512 // max(regs, 8))))
    names = subprocess.run(["c++filt"], input="\n".join(r[1]["name"] for r in rows), capture_output=True, text=True).stdout.split("\n")
    print("file vgpr agpr sgpr scratch lds waves kernel")
    for (f, k, w), n in sorted(zip(rows, names), key=lambda t: (t[0][0], t[1])):
        n = re.sub(r"^(void )?yp::|\(.*\)$", "", n).replace(" ", "")
        print(f, k["vgpr_count"], k.get("agpr_count", 0), k["sgpr_count"], k["private_segment_fixed_size"], k["group_segment_fixed_size"], w, n)


if __name__ == "__main__":
    main(sys.argv[1:])
