#!/usr/bin/env python3
"""Register, scratch and occupancy table of the FA_TRIMMED kernels (or, with --kernels centered, of the Bulyan
stage's centred-mean kernels), from hipcc's resource-usage remarks.

    hipcc ... -Rpass-analysis=kernel-resource-usage -c csrc/fa_trimmed.hip 2> remarks.log
    tools/trimmed_resources.py remarks.log [--json out.json]
    hipcc ... -Rpass-analysis=kernel-resource-usage -c csrc/fa_centered.hip 2> remarks.log
    tools/trimmed_resources.py remarks.log --kernels centered [--json out.json]

Prints one row per kernel (form, in -> out, P) and exits 1 if any kernel spills VGPRs or uses scratch.
"""
import json
import re
import subprocess
import sys


def demangle(names):
    # binutils' c++filt does not know _Float16 (DF16_): spell it as a type it does before demangling
    names = [n.replace("DF16_", "Dh") for n in names]
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return [d.replace("__fp16", "_Float16").replace("half", "_Float16") for d in out.splitlines()]


def main():
    log = open(sys.argv[1]).read()
    family = sys.argv[sys.argv.index("--kernels") + 1] if "--kernels" in sys.argv else "trimmed"
    rows, cur = [], None
    for line in log.splitlines():
        m = re.search(r"remark: .*?(Function Name|VGPRs|AGPRs|SGPRs|ScratchSize \[bytes/lane\]|"
                      r"Occupancy \[waves/SIMD\]|VGPRs Spill|SGPRs Spill): (\S+)", line)
        if not m:
            continue
        k, v = m.group(1), m.group(2)
        if k == "Function Name":
            cur = {"name": v}
            rows.append(cur)
        elif cur is not None:
            cur[k.split(" [")[0]] = int(v)
    rows = [r for r in rows if family + "_" in r["name"]]
    for r, d in zip(rows, demangle([r["name"] for r in rows])):
        m = re.search(family + r"_(vec|elem|wide)_kernel<([^,>]+), ([^,>]+)(?:, (\d+))?", d)
        r["form"], r["in"], r["out"], r["P"] = m.group(1), m.group(2), m.group(3), int(m.group(4) or 128)
    rows.sort(key=lambda r: (r["form"], r["in"], r["out"], r["P"]))
    bad = 0
    print("%-5s %-16s %-16s %4s %6s %6s %6s %8s %6s %5s" % ("form", "in", "out", "P", "VGPRs", "AGPRs", "SGPRs",
                                                             "scratch", "vspill", "occ"))
    for r in rows:
        spill = r.get("VGPRs Spill", 0)  # SGPR spills go to VGPR lanes, not to memory: listed, not counted
        bad += bool(spill or r.get("ScratchSize", 0))
        print("%-5s %-16s %-16s %4d %6d %6d %6d %8d %6d %5d" % (r["form"], r["in"], r["out"], r["P"], r["VGPRs"],
                                                                r["AGPRs"], r["SGPRs"], r.get("ScratchSize", 0), spill,
                                                                r["Occupancy"]))
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(rows, f, indent=1)
    print("%d kernels, %d with spills or scratch" % (len(rows), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
