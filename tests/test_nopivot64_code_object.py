"""CPU check of the fp64 no-pivot kernels in the shipped gfx950 code object: every one is there, none uses scratch,
and each workgroup's LDS fits the 160 KiB of a CU."""
from code_object import kernel_metadata

KERNELS = ("np64_diag_kernel", "np64_block_kernel", "np64_rank_update_kernel")


def test_nopivot64_kernels_use_no_scratch_and_fit_lds(tmp_path):
    meta = kernel_metadata(tmp_path)
    for k in KERNELS:
        found = [n for n in meta if k in n]
        assert found, k
        for n in found:
            scratch = meta[n]["private_segment_fixed_size"]
            lds = meta[n]["group_segment_fixed_size"]
            assert scratch == 0, (n, scratch)
            assert lds <= 160 * 1024, (n, lds)
    assert len([n for n in meta if "np64_diag_kernel" in n]) == 2   # block widths 64 and 128
