"""CPU check of the register-resident kernels in the shipped gfx950 code object: all 16 instances of
gj_resident_kernel are there -- T in {float, double} x L in {8, 16, 32, 64} x PIVOT in {0, 1} -- and none of them
touches scratch.  Zero is not a tuned number: a register-resident kernel that touches scratch is indexing its
registers at run time or spilling, and that is the defect this test is there to catch.  The register counts are
printed, not asserted (DESIGN.md has the table)."""
import re

from code_object import kernel_metadata

WANT = {(t, lanes, piv) for t in ("f", "d") for lanes in (8, 16, 32, 64) for piv in (0, 1)}


def _instance(name):
    m = re.search(r"gj_resident_kernelI([fd])Li(\d+)ELb([01])E", name)
    return (m.group(1), int(m.group(2)), int(m.group(3))) if m else None


def test_resident_instances_use_no_scratch(tmp_path):
    meta = {_instance(name): m for name, m in kernel_metadata(tmp_path).items() if _instance(name) is not None}
    assert set(meta) == WANT, sorted(WANT ^ set(meta))
    print("\n T   L  pivot  vgpr  sgpr")
    for (t, lanes, piv), m in sorted(meta.items()):
        print(f" {'fp32' if t == 'f' else 'fp64'} {lanes:2d}  {piv}     {m['vgpr_count']:4d}  {m['sgpr_count']:4d}")
    for inst, m in meta.items():
        assert m["private_segment_fixed_size"] == 0, (inst, m)
        assert m["vgpr_spill_count"] == 0, (inst, m)
