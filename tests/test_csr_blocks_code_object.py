"""The CSR gather's instances in the shipped gfx950 code object (metadata only, through tests/code_object.py): element
type x index type x lane class, 2 x 2 x 5 = 20 kernels, none with scratch or spilled vector registers.  Registers and
LDS are printed, not asserted."""
import re

from code_object import kernel_metadata

WANT = {(t, i, lanes) for t in ("f", "d") for i in ("i", "l") for lanes in (8, 16, 32, 64, 128)}


def _instance(name):
    m = re.search(r"csr_blocks_vkernelI([fd])([il])Li(\d+)E", name)       # <float | double, int32_t | int64_t, L>
    return (m.group(1), m.group(2), int(m.group(3))) if m else None


def test_csr_gather_instances_use_no_scratch(tmp_path):
    meta = {_instance(name): m for name, m in kernel_metadata(tmp_path).items() if _instance(name) is not None}
    assert len(WANT) == 20 and set(meta) == WANT, sorted(WANT ^ set(meta))
    print("\n T     index  lanes  vgpr  sgpr    lds")
    for (t, i, lanes), m in sorted(meta.items()):
        print(f" {'fp32' if t == 'f' else 'fp64'}  {'int32' if i == 'i' else 'int64'}  {lanes:4d}   {m['vgpr_count']:4d}  "
              f"{m['sgpr_count']:4d}  {m['group_segment_fixed_size']:6d}")
    for inst, m in meta.items():
        assert m["private_segment_fixed_size"] == 0, (inst, m)
        assert m["vgpr_spill_count"] == 0, (inst, m)
