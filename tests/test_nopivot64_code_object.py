"""CPU check of the fp64 no-pivot kernels in the shipped gfx950 code object: every one is there, none uses scratch,
and each workgroup's LDS fits the 160 KiB of a CU."""
import os
import re
import shutil
import subprocess

from gpu_matrix_inversion_amd import _lib

LLVM = "/opt/rocm/lib/llvm/bin"
KERNELS = ("np64_diag_kernel", "np64_block_kernel", "np64_rank_update_kernel")


def _kernel_metadata(tmp_path):
    """{mangled name: kernel metadata text} over every gfx950 code object of the library."""
    copy = tmp_path / os.path.basename(_lib.LIB_PATH)
    shutil.copy(_lib.LIB_PATH, copy)
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", str(copy)], check=True, capture_output=True, cwd=tmp_path)
    meta = {}
    for f in sorted(os.listdir(tmp_path)):
        if "gfx950" not in f:
            continue
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(tmp_path / f)], check=True,
                               capture_output=True, text=True).stdout
        for entry in re.split(r"\n  - \.agpr_count:", notes)[1:]:
            name = re.search(r"\n    \.name:\s+(\S+)", entry)
            if name:
                meta[name.group(1)] = entry
    return meta


def test_nopivot64_kernels_use_no_scratch_and_fit_lds(tmp_path):
    meta = _kernel_metadata(tmp_path)
    for k in KERNELS:
        found = [n for n in meta if k in n]
        assert found, k
        for n in found:
            scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta[n]).group(1))
            lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", meta[n]).group(1))
            assert scratch == 0, (n, scratch)
            assert lds <= 160 * 1024, (n, lds)
    assert len([n for n in meta if "np64_diag_kernel" in n]) == 2   # block widths 64 and 128
