#!/usr/bin/env python3
"""Per-kernel register / scratch / occupancy table of the HIP library (compiler remarks, no GPU needed).

    python tools/kernel_resources.py [--scratch] [--unit=sdqh_sort.hip] [substring ...]

--unit names the translation unit under sdqlpy_amd/csrc (default sdqh_hip.hip, the ahead-of-time kernels); SGPR spills are shown
because a kernel whose argument block overflows the SGPRs spills them to VGPR lanes, which costs registers but no memory.

A kernel that shows scratch bytes, or whose VGPR count jumped, regressed at compile time: by-value
argument structs indexed with a run-time index get copied to scratch.
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout
    return out.splitlines()


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    only_scratch = "--scratch" in sys.argv
    unit = ([a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--unit=")] or ["sdqh_hip.hip"])[-1]
    src = os.path.join(ROOT, "sdqlpy_amd", "csrc", unit)
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
           "-munsafe-fp-atomics", "-fno-gpu-rdc", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", os.path.dirname(src),
           "-Rpass-analysis=kernel-resource-usage", "-o", "/tmp/_kernel_resources_%s.so" % os.path.splitext(unit)[0], src]
    err = subprocess.run(cmd, capture_output=True, text=True).stderr
    rows, cur = [], None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith("Function Name:"):
            cur = {"name": text.split(":", 1)[1].strip()}
            rows.append(cur)
        elif cur is not None and ":" in text:
            k, v = text.split(":", 1)
            cur[k.strip()] = v.strip()
    names = demangle([r["name"] for r in rows])
    print("%-6s %-6s %-8s %-4s %-6s %-8s %-8s %s" % ("VGPR", "SGPR", "scratch", "occ", "LDS", "SGPRspl", "VGPRspl", "kernel"))
    for r, n in zip(rows, names):
        n = re.sub(r"\(.*", "", n.replace("(anonymous namespace)::", "")).replace("void sdqh::", "").replace("sdqh::", "").replace("void ", "")
        if args and not any(a in n for a in args):
            continue
        scratch = int(r.get("ScratchSize [bytes/lane]", "0"))
        if only_scratch and not scratch:
            continue
        print("%-6s %-6s %-8d %-4s %-6s %-8s %-8s %s" % (r.get("VGPRs", "?"), r.get("TotalSGPRs", "?"), scratch, r.get("Occupancy [waves/SIMD]", "?"),
                                                     r.get("LDS Size [bytes/block]", "?"), r.get("SGPRs Spill", "?"), r.get("VGPRs Spill", "?"), n))


if __name__ == "__main__":
    main()
