#!/usr/bin/env python3
"""Side-by-side kernel resource usage of two builds of interp.hip.

Each input is the compiler's output for
    hipcc <the Makefile's HIPFLAGS> -c interp.hip -Rpass-analysis=kernel-resource-usage
(`make asm` in bpftime_amd/csrc prints the same remarks).  Prints one row per
kernel with SGPRs, VGPRs, AGPRs, scratch bytes per lane, SGPR / VGPR spills,
occupancy and LDS of both builds and a `same` / `DIFF` mark, the LDS-stack
instances of k_interp (template argument BIGSTACK = false) first.  Exit
status 1 when any of those differs.

usage: resource_diff.py PARENT.txt THIS.txt
"""
import re
import subprocess
import sys

FIELDS = [("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("SGPRs Spill", "sspill"), ("VGPRs Spill", "vspill"), ("Occupancy [waves/SIMD]", "occ"),
          ("LDS Size [bytes/block]", "lds")]


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        body = m.group(1).strip()
        if body.startswith("Function Name:"):
            cur = body.split(":", 1)[1].strip()
            out[cur] = {}
            continue
        for name, key in FIELDS:
            if cur and body.startswith(name + ":"):
                out[cur][key] = body.split(":", 1)[1].strip()
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    names = sorted(set(a) | set(b))
    pretty = demangle(names)

    def lds_stack(n):  # k_interp<KIND, BIGSTACK = false, ...>
        return re.search(r"k_interp<\d+u?, false,", pretty[n]) is not None

    keys = [k for _, k in FIELDS]
    print("columns (parent | this): " + " ".join(keys))
    bad = 0
    for group, title in ((True, "LDS-stack instances of k_interp"), (False, "every other kernel")):
        print(f"\n== {title}")
        for n in names:
            if lds_stack(n) != group:
                continue
            ra, rb = a.get(n, {}), b.get(n, {})
            same = ra == rb
            bad += group and not same
            print(f"{'same' if same else 'DIFF'}  {pretty[n]}")
            print("      " + " ".join(ra.get(k, "-") for k in keys) + "  |  " + " ".join(rb.get(k, "-") for k in keys))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
