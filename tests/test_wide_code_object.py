"""CPU check of the wide workgroup-resident kernels in the shipped gfx950 code object: all 16 instances are there --
(columns per slab, rows per thread) in {(192, 40), (192, 48), (256, 56), (256, 64)} x PIVOT in {0, 1} x {gj_wide_kernel,
gj_wide_det_kernel} --, none touches scratch or spills a vector register, and each fits the register budget of its
workgroup size: a compute unit has 4 x 512 registers per lane, so 16 waves (1024 threads) leave 128 per thread and 12
waves (768 threads) 168 (512 / 3 rounded down to the allocation granule of 8); an instance above that cannot be
launched.  The register counts are printed, not otherwise asserted (DESIGN.md section 17 has the table)."""
import os
import re
import subprocess

from code_object import LLVM, kernel_metadata
from wide_cases import CLASSES

WANT = {(det, c, rpt, piv) for det in (0, 1) for c, rpt in CLASSES for piv in (0, 1)}
BUDGET = {768: 168, 1024: 128}   # threads -> vector + accumulation registers per thread


def _instance(name):
    m = re.search(r"gj_wide_(det_)?kernelILi(\d+)ELi(\d+)ELb([01])E", name)
    return (int(bool(m.group(1))), int(m.group(2)), int(m.group(3)), int(m.group(4))) if m else None


def _agpr_counts(tmp_path):
    """{kernel name: .agpr_count}: the key kernel_metadata splits the notes at."""
    out = {}
    for f in sorted(os.listdir(tmp_path)):
        if "gfx950" not in f:
            continue
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(tmp_path / f)], check=True, capture_output=True,
                               text=True).stdout
        for entry in re.split(r"\n  - (?=\.agpr_count:)", notes)[1:]:
            name = re.search(r"\n    \.name:\s+(\S+)", entry)
            count = re.match(r"\.agpr_count:\s+(\d+)", entry)
            if name and count:
                out[name.group(1)] = int(count.group(1))
    return out


def test_wide_instances_fit_their_workgroup(tmp_path):
    all_meta = kernel_metadata(tmp_path)
    agpr = _agpr_counts(tmp_path)
    meta = {_instance(name): dict(m, agpr_count=agpr[name]) for name, m in all_meta.items() if _instance(name) is not None}
    assert set(meta) == WANT, sorted(WANT ^ set(meta))
    print("\n det  C  RPT pivot  vgpr  agpr  sgpr  sgpr spills   lds")
    for (det, c, rpt, piv), m in sorted(meta.items()):
        print(f"  {det}  {c:3d} {rpt:3d}  {piv}     {m['vgpr_count']:4d}  {m['agpr_count']:4d}  {m['sgpr_count']:4d}  "
              f"{m['sgpr_spill_count']:4d}        {m['group_segment_fixed_size']:5d}")
    for inst, m in meta.items():
        threads = 4 * inst[1]
        assert m["max_flat_workgroup_size"] == threads, (inst, m)
        assert m["private_segment_fixed_size"] == 0, (inst, m)
        assert m["vgpr_spill_count"] == 0, (inst, m)
        assert m["vgpr_count"] + m["agpr_count"] <= BUDGET[threads], (inst, m)
        assert m["group_segment_fixed_size"] < 16 * 1024, (inst, m)
