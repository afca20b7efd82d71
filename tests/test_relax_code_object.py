"""CPU check of the relaxation kernels in the shipped gfx950 code object: the forty instances of relax_stored_vkernel
are there -- T in {float, double} x index in {int32_t, int64_t} x L in {8, 16, 32, 64, 128} lanes per member x {the
residual alone, the fused sweep} -- and none touches scratch or spills a register; the residual-only instances use no
LDS at all, the sweep instances leave room for three workgroups per CU.  The register and LDS counts are printed, not
asserted (DESIGN.md section 23 has the table).  Metadata only."""
import re

from code_object import kernel_metadata

WANT = {(t, i, lanes, sweep) for t in "fd" for i in "il" for lanes in (8, 16, 32, 64, 128) for sweep in (0, 1)}


def _instance(name):
    m = re.search(r"relax_stored_vkernelI([fd])([il])Li(\d+)ELb([01])E", name)   # <T, I, L, kSweep>
    return (m.group(1), m.group(2), int(m.group(3)), int(m.group(4))) if m else None


def test_relax_instances_use_no_scratch(tmp_path):
    meta = kernel_metadata(tmp_path)
    named = [name for name in meta if "relax_stored_vkernel" in name]
    inst = {_instance(name): meta[name] for name in named}
    assert len(named) == len(WANT) == 40 and set(inst) == WANT, sorted(WANT ^ set(inst), key=str)
    print("\n T     index  lanes  form      vgpr  sgpr    lds")
    for (t, i, lanes, sweep), m in sorted(inst.items()):
        print(f" {'fp32' if t == 'f' else 'fp64'}  {'int32' if i == 'i' else 'int64'}  {lanes:4d}   "
              f"{'sweep   ' if sweep else 'residual'}  {m['vgpr_count']:4d}  {m['sgpr_count']:4d}  "
              f"{m['group_segment_fixed_size']:6d}")
    for key, m in inst.items():
        assert m["private_segment_fixed_size"] == 0, (key, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (key, m)
        assert m["group_segment_fixed_size"] <= 160 * 1024 // 3, (key, m)   # several workgroups per CU
        if not key[3]:
            assert m["group_segment_fixed_size"] == 0, (key, m)
