"""CPU check of the kernels of the determinant above order 128 in the shipped gfx950 code object: every one is there --
the det twins of the sweep and of the fp64 blocked step kernel in every instance their plain kernels have, the input
scan, the pivot gather, the row-map parity and the finish kernel -- and none uses scratch or spills a register.  A det
twin's registers and LDS are those of its plain kernel, or within the few registers the extra store needs; the plain
step kernels, which share their twin's body, use no scratch either and no more vector registers than the twin."""
from code_object import kernel_metadata

# kernel name fragment -> number of instances
NEW_KERNELS = {
    "gj_sweep_step_det_kernel": 16,    # float / double x 4, 8, 16, 32 rows per workgroup x pivoting on / off
    "b64_panel_step_det_kernel": 6,    # block widths 64, 128, 256 x 8 / 32 rows per workgroup
    "det_scan_kernel": 2,              # float, double
    "det_gather_kernel": 1,
    "det_parity_kernel": 1,
    "det_finish_kernel": 4,            # float / double x pivoting on / off
}
TWINS = {"gj_sweep_step_det_kernel": "gj_sweep_step_kernel", "b64_panel_step_det_kernel": "b64_panel_step_kernel"}


def test_det_large_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    meta = kernel_metadata(tmp_path)
    for k, count in NEW_KERNELS.items():
        found = [n for n in meta if k in n]
        assert len(found) == count, (k, found)
        for n in found:
            m = meta[n]
            assert m["private_segment_fixed_size"] == 0, (n, m)
            assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (n, m)
            assert m["group_segment_fixed_size"] <= 64 * 1024, (n, m)
    for twin, plain in TWINS.items():
        for n, t in _plain_and_twin(meta, plain, twin):
            a, b = meta[n], meta[t]
            assert b["group_segment_fixed_size"] == a["group_segment_fixed_size"], (n, a, b)
            assert b["vgpr_count"] <= a["vgpr_count"] + 8, (n, a, b)


def _plain_and_twin(meta, plain, twin):
    """[(plain instance, its twin)], mangled names, for every instance of the plain kernel."""
    plain_instances = [n for n in meta if plain in n]
    assert len(plain_instances) == NEW_KERNELS[twin]
    pairs = []
    for n in plain_instances:
        # the twin's mangled name: the plain kernel's with three more parameters (pointer, size_t, int pointer)
        t = [x for x in meta if x.startswith(n.replace(plain, twin).replace(str(len(plain)) + twin, str(len(twin)) + twin))]
        assert len(t) == 1, (n, t)
        pairs.append((n, t[0]))
    return pairs


def test_plain_step_kernels_use_no_scratch_and_no_more_registers_than_their_twins(tmp_path):
    """A plain step kernel and its twin are one function body (sweep_step, b64_step) with the det lines compiled out of
    the plain one: it has no scratch and no spills either, and never needs more vector registers than the twin."""
    meta = kernel_metadata(tmp_path)
    for twin, plain in TWINS.items():
        for n, t in _plain_and_twin(meta, plain, twin):
            m = meta[n]
            assert m["private_segment_fixed_size"] == 0, (n, m)
            assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (n, m)
            assert m["vgpr_count"] <= meta[t]["vgpr_count"], (n, m, meta[t])
