"""CPU check of the workgroup-resident kernels in the shipped gfx950 code object: all 16 instances of
gj_workgroup_kernel are there -- T in {float, double} x RPT in {40, 48, 56, 64} x PIVOT in {0, 1} -- and none of
them touches scratch.  Zero is not a tuned number: the matrix lives in registers, and a kernel that touches scratch is
indexing them at run time (the pivot slot is a run-time value) or spilling, which is the defect this test is there
to catch.  The register counts are printed, not asserted (DESIGN.md has the table)."""
import os
import re
import shutil
import subprocess

from gpu_matrix_inversion_amd import _lib

LLVM = "/opt/rocm/lib/llvm/bin"
WANT = {(t, rpt, piv) for t in ("f", "d") for rpt in (40, 48, 56, 64) for piv in (0, 1)}


def _instance(name):
    m = re.search(r"gj_workgroup_kernelI([fd])Li(\d+)ELb([01])E", name)
    return (m.group(1), int(m.group(2)), int(m.group(3))) if m else None


def test_workgroup_instances_use_no_scratch(tmp_path):
    copy = tmp_path / os.path.basename(_lib.LIB_PATH)
    shutil.copy(_lib.LIB_PATH, copy)
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", str(copy)], check=True, capture_output=True, cwd=tmp_path)
    meta = {}
    for f in sorted(os.listdir(tmp_path)):
        if "gfx950" not in f:
            continue
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(tmp_path / f)], check=True, capture_output=True,
                               text=True).stdout
        for entry in re.split(r"\n  - \.agpr_count:", notes)[1:]:
            name = re.search(r"\n    \.name:\s+(\S+)", entry)
            if name and _instance(name.group(1)) is not None:
                meta[_instance(name.group(1))] = {
                    key: int(re.search(r"\.%s:\s+(\d+)" % key, entry).group(1))
                    for key in ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_count",
                                "group_segment_fixed_size")}
    assert set(meta) == WANT, sorted(WANT ^ set(meta))
    print("\n T    RPT pivot  vgpr  sgpr  lds")
    for (t, rpt, piv), m in sorted(meta.items()):
        print(f" {'fp32' if t == 'f' else 'fp64'} {rpt:3d}  {piv}     {m['vgpr_count']:4d}  {m['sgpr_count']:4d}  "
              f"{m['group_segment_fixed_size']:5d}")
    for inst, m in meta.items():
        assert m["private_segment_fixed_size"] == 0, (inst, m)
        assert m["vgpr_spill_count"] == 0, (inst, m)
