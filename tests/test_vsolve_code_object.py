"""CPU check of the variable-size solve kernels in the shipped gfx950 code object: all 32 instances are there --
gj_resident_solve_vkernel (T in {float, double} x L in {8, 16, 32, 64} x PIVOT in {0, 1}) and gj_workgroup_solve_vkernel
(RPT in {40, 48, 56, 64}) -- and none of them touches scratch or spills: the member look-up, the three leading
dimensions and the per-group order must not push a register array into memory.  The register counts are printed, not
asserted (DESIGN.md section 14 has the table)."""
import re

from code_object import kernel_metadata

WANT = {(kern, t, size, piv) for kern, sizes in (("resident", (8, 16, 32, 64)), ("workgroup", (40, 48, 56, 64)))
        for t in ("f", "d") for size in sizes for piv in (0, 1)}


def _instance(name):
    m = re.search(r"gj_(resident|workgroup)_solve_vkernelI([fd])Li(\d+)ELb([01])E", name)
    return (m.group(1), m.group(2), int(m.group(3)), int(m.group(4))) if m else None


def test_vsolve_instances_use_no_scratch(tmp_path):
    meta = {_instance(name): m for name, m in kernel_metadata(tmp_path).items() if _instance(name) is not None}
    assert len(WANT) == 32 and set(meta) == WANT, sorted(WANT ^ set(meta))
    print("\n kernel     T     size pivot  vgpr  sgpr   lds")
    for (kern, t, size, piv), m in sorted(meta.items()):
        print(f" {kern:9s}  {'fp32' if t == 'f' else 'fp64'}  {size:3d}  {piv}     {m['vgpr_count']:4d}  "
              f"{m['sgpr_count']:4d}  {m['group_segment_fixed_size']:5d}")
    for inst, m in meta.items():
        assert m["private_segment_fixed_size"] == 0, (inst, m)
        assert m["vgpr_spill_count"] == 0, (inst, m)
