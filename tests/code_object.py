"""The kernel metadata of the shipped gfx950 code object, for the CPU tests that check instance lists, scratch, spills
and LDS (no pytest in here: the test files import what they need)."""
import os
import re
import shutil
import subprocess

from gpu_matrix_inversion_amd import _lib

LLVM = "/opt/rocm/lib/llvm/bin"


def kernel_metadata(tmp_path):
    """{mangled kernel name: {metadata key: value}} over every gfx950 code object of the library, the integer-valued
    keys of the kernel's note entry (private_segment_fixed_size, vgpr_count, vgpr_spill_count, sgpr_count,
    group_segment_fixed_size, ...).  `tmp_path`: an empty directory the code objects are extracted into."""
    copy = tmp_path / os.path.basename(_lib.LIB_PATH)
    shutil.copy(_lib.LIB_PATH, copy)
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", str(copy)], check=True, capture_output=True, cwd=tmp_path)
    meta = {}
    for f in sorted(os.listdir(tmp_path)):
        if "gfx950" not in f:
            continue
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(tmp_path / f)], check=True, capture_output=True,
                               text=True).stdout
        for entry in re.split(r"\n  - \.agpr_count:", notes)[1:]:
            name = re.search(r"\n    \.name:\s+(\S+)", entry)
            if name:
                meta[name.group(1)] = {k: int(v) for k, v in re.findall(r"\n    \.(\w+):\s+(\d+)[ \t]*(?=\n|$)", entry)}
    return meta
