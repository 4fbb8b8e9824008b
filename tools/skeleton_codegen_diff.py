"""Does an edit of the kernel headers change the gfx950 code?  Compiles, for a base revision and for the working tree:
  * the ahead-of-time units that include sdqh_kernels.hpp only: device-side preprocessed text (hipcc -E -P --cuda-device-only);
  * sdqh_x.hip (includes sdqh_xkernels.hpp too) and every kept kernel source under sdqlpy_amd/jit_recipes/: device assembly
    (-S --cuda-device-only) with the options the library hands to hiprtc; the ahead-of-time kernels stay uninstantiated templates
    as under hiprtc (SDQH_DECLS_ONLY);
and reports per unit "identical" or the diff.  Only lines naming the per-compilation __hip_cuid_<hash> symbol may differ.
Needs hipcc and git; no GPU, no built library.
    python tools/skeleton_codegen_diff.py --base HEAD [--jobs 8] [--out profiles/skeleton_cleanup_codegen.txt]
"""
import argparse
import difflib
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRE_UNITS = ["sdqh_hip.hip", "sdqh_codes.hip", "sdqh_aux.hip", "sdqh_sort.hip", "sdqh_extrema.hip"]
INC = ["-I", "include", "-I", os.path.join("sdqlpy_amd", "csrc")]         # relative: the same text in both trees
RTC = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-munsafe-fp-atomics"]
PRE = ["hipcc", "-E", "-P", "--offload-arch=gfx950", "--cuda-device-only", "-std=c++17"] + INC
ASM = ["hipcc"] + RTC + ["--cuda-device-only", "-S"] + INC
RESOURCES = re.compile(r"\.(sgpr_count|vgpr_count|agpr_count|group_segment_fixed_size|private_segment_fixed_size):\s*(\d+)")


def run(cmd, cwd):
    p = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        raise RuntimeError("%s (in %s)\n%s" % (" ".join(cmd), cwd, p.stderr))
    return [l for l in p.stdout.splitlines() if "__hip_cuid_" not in l]


def compare(job):
    label, cmd, base, new = job
    a, b = run(cmd, base), run(cmd, new)
    text = "\n".join(b)
    res = " ".join("%s=%s" % kv for kv in sorted(set(RESOURCES.findall(text)))) if "-S" in cmd else ""
    if a == b:
        return label, True, "identical  (%d lines)" % len(b), res
    return label, False, "DIFFERS\n" + "\n".join(list(difflib.unified_diff(a, b, "base", "tree", lineterm="", n=2))[:200]), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", default="HEAD")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as base:
        tar = subprocess.run(["git", "archive", args.base, "include", "sdqlpy_amd/csrc", "sdqlpy_amd/jit_recipes"], cwd=ROOT, stdout=subprocess.PIPE, check=True)
        subprocess.run(["tar", "-x", "-C", base], input=tar.stdout, check=True)
        jobs = [("preprocessed  " + u, PRE + [os.path.join("sdqlpy_amd", "csrc", u)], base, ROOT) for u in PRE_UNITS]
        jobs.append(("assembly      sdqh_x.hip", ASM + ["-o", "-", os.path.join("sdqlpy_amd", "csrc", "sdqh_x.hip")], base, ROOT))
        for path in sorted(glob.glob(os.path.join(ROOT, "sdqlpy_amd", "jit_recipes", "*.hip"))):
            rel = os.path.relpath(path, ROOT)
            jobs.append(("assembly      " + rel, ASM + ["-DSDQH_DECLS_ONLY", "-o", "-", rel], base, ROOT))
        with ThreadPoolExecutor(args.jobs) as pool:
            results = list(pool.map(compare, jobs))
    rev = subprocess.run(["git", "rev-parse", "--short", args.base], cwd=ROOT, stdout=subprocess.PIPE, text=True).stdout.strip()
    lines = ["# gfx950 code of the working tree's kernel headers against %s (%s): tools/skeleton_codegen_diff.py" % (args.base, rev),
             "# preprocessed: " + " ".join(PRE) + " <unit>", "# assembly:     " + " ".join(ASM) + " [-DSDQH_DECLS_ONLY] -o - <source>",
             "# lines naming __hip_cuid_<hash> are left out of both sides; resources are the kernel's own metadata in the tree's assembly", ""]
    for label, same, verdict, res in results:
        lines.append("%-58s %s%s" % (label, verdict, ("   " + res) if res else ""))
    lines += ["", "%d of %d identical" % (sum(1 for r in results if r[1]), len(results))]
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    sys.stdout.write(text)
    return 0 if all(r[1] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
