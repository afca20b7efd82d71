"""The block finder's instances in the shipped gfx950 code object (metadata only, through tests/code_object.py): the
pattern compare per index type and the four kernels behind it, none with scratch or spilled registers.  Registers and
LDS are printed, not asserted."""
import re

from code_object import kernel_metadata

WANT = {"nat<int32>", "nat<int64>", "runs", "sv", "chain", "mark"}


def _instance(name):
    m = re.search(r"csr_find_(nat|runs|sv|chain|mark)_kernel(?:I([il])E)?", name)
    if not m:
        return None
    return m.group(1) + ({"i": "<int32>", "l": "<int64>"}[m.group(2)] if m.group(2) else "")


def test_block_finder_instances_use_no_scratch(tmp_path):
    meta = {_instance(name): m for name, m in kernel_metadata(tmp_path).items() if _instance(name) is not None}
    assert set(meta) == WANT, sorted(WANT ^ set(meta))
    print("\n kernel       vgpr  sgpr    lds")
    for inst, m in sorted(meta.items()):
        print(f" {inst:11s}  {m['vgpr_count']:4d}  {m['sgpr_count']:4d}  {m['group_segment_fixed_size']:6d}")
    for inst, m in meta.items():
        assert m["private_segment_fixed_size"] == 0, (inst, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (inst, m)
