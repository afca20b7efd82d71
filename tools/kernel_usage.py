#!/usr/bin/env python3
"""Print a per-kernel resource table (VGPR/SGPR/scratch/LDS/occupancy) for the HIP sources.

    python tools/kernel_usage.py [--filter NAME] [source.hip ...]

Without sources: every source of csrc/Makefile.  --filter keeps the kernels whose demangled name contains NAME.
"""
import argparse, re, subprocess, os
here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpu_matrix_inversion_amd", "csrc")
mk = open(os.path.join(here, "Makefile")).read()
var = lambda name, op: re.search(rf"^{name}\s*{op}\s*(.*?)(?<!\\)$", mk, re.M | re.S).group(1).replace("\\\n", " ").split()
ap = argparse.ArgumentParser()
ap.add_argument("--filter", default="")
ap.add_argument("files", nargs="*")
args = ap.parse_args()
# exactly the flags of csrc/Makefile (a different flag set gives different register allocation)
flags = [fl.replace("$(ARCH)", "gfx950") for fl in var("FLAGS", r"\?=")]
for f in args.files or var("SRCS", ":="):
    out = subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["-c", f, "-o", "/dev/null",
                          "-Rpass-analysis=kernel-resource-usage"], cwd=here, capture_output=True, text=True).stderr
    cur = None
    rows = {}
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            cur = re.sub(r"\(.*", "", cur)
            rows[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", line)
        if m and cur:
            rows[cur][m.group(1).strip()] = int(m.group(2))
    for k, v in rows.items():
        if args.filter in k:
            print(f"{k:60s} vgpr={v.get('VGPRs',-1):4d} agpr={v.get('AGPRs',-1):3d} sgpr={v.get('TotalSGPRs',-1):4d} scratch={v.get('ScratchSize',-1):5d} vspill={v.get('VGPRs Spill',-1):4d} lds={v.get('LDS Size',-1):6d} occ={v.get('Occupancy',-1)}")
