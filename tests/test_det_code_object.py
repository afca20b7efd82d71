"""CPU check of the determinant kernels in the shipped gfx950 code object: all 64 instances are there --
gj_resident_det_kernel / gj_resident_det_vkernel (T in {float, double} x L in {8, 16, 32, 64} x PIVOT in {0, 1}) and
gj_workgroup_det_kernel / gj_workgroup_det_vkernel (RPT in {40, 48, 56, 64}) -- and none of them touches scratch or
spills: the three words of the accumulator must not push a register array into memory.  The register counts are
printed, not asserted (DESIGN.md section 12 has the table)."""
import os
import re
import shutil
import subprocess

from gpu_matrix_inversion_amd import _lib

LLVM = "/opt/rocm/lib/llvm/bin"
WANT = {(kern, var, t, size, piv) for kern, sizes in (("resident", (8, 16, 32, 64)), ("workgroup", (40, 48, 56, 64)))
        for var in ("kernel", "vkernel") for t in ("f", "d") for size in sizes for piv in (0, 1)}


def _instance(name):
    m = re.search(r"gj_(resident|workgroup)_det_(v?kernel)I([fd])Li(\d+)ELb([01])E", name)
    return (m.group(1), m.group(2), m.group(3), int(m.group(4)), int(m.group(5))) if m else None


def test_det_instances_use_no_scratch(tmp_path):
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
    assert len(WANT) == 64 and set(meta) == WANT, sorted(WANT ^ set(meta))
    print("\n kernel     form     T     size pivot  vgpr  sgpr   lds")
    for (kern, var, t, size, piv), m in sorted(meta.items()):
        print(f" {kern:9s}  {var:7s}  {'fp32' if t == 'f' else 'fp64'}  {size:3d}  {piv}     {m['vgpr_count']:4d}  "
              f"{m['sgpr_count']:4d}  {m['group_segment_fixed_size']:5d}")
    for inst, m in meta.items():
        assert m["private_segment_fixed_size"] == 0, (inst, m)
        assert m["vgpr_spill_count"] == 0, (inst, m)
