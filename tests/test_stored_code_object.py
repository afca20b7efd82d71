"""CPU check of the stored-inverse kernels in the shipped gfx950 code object: the three families are there --
block_stats_vkernel, store_vkernel and apply_stored_vkernel, each T in {float, double} x L in {8, 16, 32, 64, 128}
lanes per member, thirty instances -- and no other kernel carries one of those names; none touches scratch or spills a
vector register (the parked tile of the apply instances and their accumulators must stay in registers), and LDS leaves
room for three workgroups per CU.  The register and LDS counts are printed, not asserted (DESIGN.md section 20 has the
table).  Metadata only."""
import re

from code_object import kernel_metadata

FAMILIES = ("block_stats_vkernel", "store_vkernel", "apply_stored_vkernel")
WANT = {(f, t, lanes) for f in FAMILIES for t in ("f", "d") for lanes in (8, 16, 32, 64, 128)}


def _instance(name):
    m = re.search(r"\d+(block_stats_vkernel|store_vkernel|apply_stored_vkernel)I([fd])Li(\d+)E", name)
    return (m.group(1), m.group(2), int(m.group(3))) if m else None


def test_stored_instances_use_no_scratch(tmp_path):
    meta = kernel_metadata(tmp_path)
    named = [name for name in meta if any(f in name for f in FAMILIES)]
    inst = {_instance(name): meta[name] for name in named}
    assert len(named) == len(WANT) == 30 and set(inst) == WANT, sorted(WANT ^ set(inst), key=str)
    print("\n family                T     lanes  vgpr  sgpr    lds")
    for (f, t, lanes), m in sorted(inst.items()):
        print(f" {f:21s} {'fp32' if t == 'f' else 'fp64'}  {lanes:4d}   {m['vgpr_count']:4d}  {m['sgpr_count']:4d}  "
              f"{m['group_segment_fixed_size']:6d}")
    for key, m in inst.items():
        assert m["private_segment_fixed_size"] == 0, (key, m)
        assert m["vgpr_spill_count"] == 0, (key, m)
        assert m["group_segment_fixed_size"] <= 160 * 1024 // 3, (key, m)   # several workgroups per CU
