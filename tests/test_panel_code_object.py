"""CPU checks of the panel kernels in the shipped gfx950 code object: every instance is there, the instances with
three rows per lane use no scratch, no instance uses more scratch than it did before they were added, the DPP
self-test kernel holds the instructions it is there to test; and the tie inputs of tests/test_gpu_panel_ties.py are inverted by the oracle with status 0."""
import os
import re
import shutil
import subprocess

import pytest

from gpu_matrix_inversion_amd import _lib
from panel_tie_cases import CASES, TIE_VALUE, oracle_inverse, tie_matrix

LLVM = "/opt/rocm/lib/llvm/bin"

# private_segment_fixed_size (bytes of scratch per lane) of the instances that use any; every other instance uses none.
# Keys: <NT, RPT, W, FUSED> of gj_subpanel_kernel, "multi" = gj_panel_multi_kernel<16>.
SCRATCH = {
    (1024, 16, 4, 0): 92, (1024, 1, 32, 1): 52, (1024, 2, 32, 0): 16, (1024, 2, 32, 1): 276, (1024, 4, 16, 0): 16,
    (1024, 8, 8, 0): 24, (512, 4, 32, 0): 36, (512, 4, 32, 1): 92, "multi": 12,
}
THREE_ROWS = [(1024, 3, 4, 0), (1024, 3, 8, 0), (1024, 3, 16, 0)]
N_INSTANCES = 57 + len(THREE_ROWS) + 1
SELFTEST = "_ZN4mi3219dpp_selftest_kernelEPKjPj"


def _instance(name):
    m = re.search(r"gj_subpanel_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])E", name)
    if m:
        return tuple(int(v) for v in m.groups())
    return "multi" if "gj_panel_multi_kernelILi16E" in name else None


def test_panel_instances_and_their_scratch(tmp_path):
    copy = tmp_path / os.path.basename(_lib.LIB_PATH)
    shutil.copy(_lib.LIB_PATH, copy)
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", str(copy)], check=True, capture_output=True, cwd=tmp_path)
    meta = {}
    dpp = {"v_fmac_f32_dpp": 0, "v_cndmask_b32_dpp": 0}
    for f in sorted(os.listdir(tmp_path)):
        if "gfx950" not in f:
            continue
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--disassemble-symbols=" + SELFTEST,
                              str(tmp_path / f)], check=True, capture_output=True, text=True).stdout
        for op in dpp:
            dpp[op] += len(re.findall(op + r" .* row_newbcast:\d+ row_mask:0xf bank_mask:0xf", dis))
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(tmp_path / f)], check=True, capture_output=True,
                               text=True).stdout
        for entry in re.split(r"\n  - \.agpr_count:", notes)[1:]:
            name = re.search(r"\n    \.name:\s+(\S+)", entry)
            if name and _instance(name.group(1)) is not None:
                meta[_instance(name.group(1))] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", entry).group(1))
    assert dpp == {"v_fmac_f32_dpp": 16, "v_cndmask_b32_dpp": 16}, dpp
    assert len(meta) == N_INSTANCES, sorted(map(str, meta))
    for inst in THREE_ROWS:
        assert meta[inst] == 0, (inst, meta[inst])
    for inst, scratch in meta.items():
        assert scratch <= SCRATCH.get(inst, 0), (inst, scratch)


@pytest.mark.parametrize("n,deltas", CASES)
def test_oracle_inverts_the_tie_inputs(oracle, n, deltas):
    a, pairs = tie_matrix(n, deltas, 77_000 + n)
    assert len(pairs) >= 8
    for j, (r1, r2) in pairs.items():
        assert abs(a[r1, j]) == abs(a[r2, j]) == TIE_VALUE and not a[r1, :j].any() and not a[r2, :j].any()
    x, info = oracle_inverse(oracle, a, n)
    assert info["status"] == 0
    assert oracle.residual_inf(a, x, n) < 1e-2
