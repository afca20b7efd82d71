"""CPU check of the apply kernels in the shipped gfx950 code object: the ten instances are there -- apply_vkernel, T in
{float, double} x L in {8, 16, 32, 64, 128} lanes per member -- and none of them touches scratch or spills: the
prefetched tile and the accumulators must stay in registers.  The register and LDS counts are printed, not asserted
(DESIGN.md section 15 has the table).  Metadata only."""
import re

from code_object import kernel_metadata

WANT = {(t, lanes) for t in ("f", "d") for lanes in (8, 16, 32, 64, 128)}


def _instance(name):
    m = re.search(r"apply_vkernelI([fd])Li(\d+)E", name)
    return (m.group(1), int(m.group(2))) if m else None


def test_apply_instances_use_no_scratch(tmp_path):
    meta = {_instance(name): m for name, m in kernel_metadata(tmp_path).items() if _instance(name) is not None}
    assert len(WANT) == 10 and set(meta) == WANT, sorted(WANT ^ set(meta))
    print("\n T     lanes  vgpr  sgpr    lds")
    for (t, lanes), m in sorted(meta.items()):
        print(f" {'fp32' if t == 'f' else 'fp64'}  {lanes:4d}   {m['vgpr_count']:4d}  {m['sgpr_count']:4d}  "
              f"{m['group_segment_fixed_size']:6d}")
    for inst, m in meta.items():
        assert m["private_segment_fixed_size"] == 0, (inst, m)
        assert m["vgpr_spill_count"] == 0, (inst, m)
        assert m["group_segment_fixed_size"] <= 160 * 1024 // 3, (inst, m)   # several workgroups per CU
