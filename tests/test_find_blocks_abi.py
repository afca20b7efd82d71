"""CPU checks of the block finder's host side (no device), following tests/test_csr_blocks_abi.py: the names in their
header (include/mat_inv_32_csr_find.h), the binding and the library; the work-bytes query; the argument guards of the
device call, which answer before a context is touched; and the pure argument checks of the Python side."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

from gpu_matrix_inversion_amd import _lib, api

NEW_SYMBOLS = ("mi32_csr_find_blocks_work_bytes", "mi32_csr_find_blocks_device", "mi32_csr_find_blocks_chunk_rows")
CPU = torch.device("cpu")


def work_bytes(n):
    size = ctypes.c_size_t(0)
    rc = _lib.load().mi32_csr_find_blocks_work_bytes(n, ctypes.byref(size))
    return rc, size.value


def test_names_in_header_binding_and_library():
    hdr = open(os.path.join(ROOT, "include", "mat_inv_32_csr_find.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    assert sorted(re.findall(r"\b(mi32_[a-z0-9_]+)\s*\(", code)) == sorted(NEW_SYMBOLS) == sorted(_lib.CSR_FIND_ABI_SYMBOLS)
    assert '#include "mat_inv_32_c.h"' in code
    for sym in NEW_SYMBOLS:
        assert sym not in _lib.C_ABI_SYMBOLS and sym not in _lib.CSR_ABI_SYMBOLS
        assert getattr(lib, sym).restype is ctypes.c_int
    assert re.search(r"int mi32_csr_find_blocks_work_bytes\(long long n, size_t \*bytes\);", code)
    assert re.search(r"int mi32_csr_find_blocks_device\(mi32_handle_t h, long long n, const void \*d_row_ptr, "
                     r"const void \*d_col,\s*int index_bytes, int max_order, int agglomerate,\s*"
                     r"unsigned char \*d_start, void \*d_work, size_t work_bytes\);", code)
    assert lib.mi32_csr_find_blocks_device.argtypes == [
        ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    assert lib.mi32_version() >= 147


def test_work_bytes_is_monotone_and_linear():
    lib = _lib.load()
    assert lib.mi32_csr_find_blocks_work_bytes(1, None) == _lib.MI32_BAD_SHAPE
    for n in (0, -1, -2**40):
        assert work_bytes(n)[0] == _lib.MI32_BAD_SHAPE, n
    chunk = lib.mi32_csr_find_blocks_chunk_rows()
    assert chunk == api.find_blocks_chunk_rows() and chunk > 8 * 128
    sizes = [1, 2, 127, 128, 129, chunk - 1, chunk, chunk + 1, 3 * chunk + 97, 10**5, 2**20, 10**7, 2**31 + 5, 10**10]
    got = []
    for n in sizes:
        rc, b = work_bytes(n)
        assert rc == _lib.MI32_OK and b > 0 and b % 16 == 0, n
        assert api.find_blocks_work_bytes(n) == b
        got.append(b)
    assert all(a <= b for a, b in zip(got, got[1:]))
    for n, b in zip(sizes, got):                      # the documented 2.1 bytes per row, and one chunk's worth at most
        assert 2 * n <= b <= 2.2 * n + 2.2 * chunk, (n, b)


def test_guards_answer_without_a_device():
    lib = _lib.load()
    fn = lib.mi32_csr_find_blocks_device
    # no entry point reads the context before its arguments are accepted: zeros stand in for it
    fake_h = ctypes.create_string_buffer(4096)
    h = ctypes.cast(fake_h, ctypes.c_void_p)
    rp, col, start, work = (ctypes.c_void_p(256 * k) for k in range(1, 5))      # never dereferenced by a refused call
    n = 1000
    need = work_bytes(n)[1]
    bad = _lib.MI32_BAD_SHAPE
    assert fn(None, n, rp, col, 4, 32, 1, start, work, need) == bad            # null handle
    assert fn(h, n, None, col, 4, 32, 1, start, work, need) == bad             # null row_ptr
    assert fn(h, n, rp, None, 8, 32, 1, start, work, need) == bad              # null col
    assert fn(h, n, rp, col, 4, 32, 0, None, work, need) == bad                # null start
    assert fn(h, n, rp, col, 4, 32, 1, start, None, need) == bad               # null work
    for rows in (0, -1, -2**33):
        assert fn(h, rows, rp, col, 4, 32, 1, start, work, need) == bad, rows
    for index_bytes in (0, 2, 5, 16, -4):
        assert fn(h, n, rp, col, index_bytes, 32, 1, start, work, need) == bad, index_bytes
    for max_order in (0, -1, 129, 256, 2**20):
        assert fn(h, n, rp, col, 8, max_order, 1, start, work, need) == bad, max_order
    for short in (0, 1, need - 1):
        assert fn(h, n, rp, col, 4, 32, 1, start, work, short) == bad, short
    assert fn(h, n, rp, col, 4, 32, 1, start, ctypes.c_void_p(1024 + 8), need) == bad    # work not 16-byte aligned


def pattern(n=6, dtype=torch.int64):
    crow = torch.arange(n + 1, dtype=dtype)
    return crow, torch.arange(n, dtype=dtype)


def test_python_checks_raise_value_error():
    crow, col = pattern()
    assert api.check_csr_pattern(CPU, crow, col) == 6
    parts = api.csr_pattern_parts((crow, col, None))
    assert len(parts) == 2 and parts[0] is crow and parts[1] is col
    vals = torch.ones(6)
    assert api.csr_pattern_parts((crow, col, vals))[1] is col
    sp = torch.sparse_csr_tensor(crow, col, vals, size=(6, 6))
    assert torch.equal(api.csr_pattern_parts(sp)[0], crow)
    for bad in ((crow, col), (crow, None, None), "csr", torch.eye(3), (crow.numpy(), col.numpy(), None),
                torch.sparse_csr_tensor(crow, col, vals, size=(6, 7))):
        with pytest.raises(ValueError):
            api.csr_pattern_parts(bad)
    for c, k in ((crow.float(), col), (crow, col.int()), (crow[::2], col), (crow[:1], col), (crow.reshape(1, -1), col),
                 (crow, col.reshape(2, 3))):
        with pytest.raises(ValueError):
            api.check_csr_pattern(CPU, c, k)
    with pytest.raises(ValueError):
        api.check_csr_pattern(torch.device("meta"), crow, col)
    assert api.check_find_blocks_args(32, True) == (32, True)
    assert api.check_find_blocks_args(np.int32(128), np.bool_(False)) == (128, False)
    for max_order, agglomerate in ((0, True), (129, True), (-3, False), (32.0, True), (True, True), ("32", True),
                                   (32, 1), (32, None)):
        with pytest.raises(ValueError):
            api.check_find_blocks_args(max_order, agglomerate)
    out = api.check_block_starts_out(crow, col, None, 6)
    assert out.dtype == torch.uint8 and out.shape == (6,)
    assert api.check_block_starts_out(crow, col, out, 6) is out
    alias = col.view(torch.uint8)[:6]
    for bad in (torch.zeros(6, dtype=torch.int8), torch.zeros(5, dtype=torch.uint8), torch.zeros(7, dtype=torch.uint8),
                torch.zeros(12, dtype=torch.uint8)[::2], torch.zeros(2, 3, dtype=torch.uint8),
                torch.zeros(6, dtype=torch.uint8, device="meta"), alias, crow.view(torch.uint8)[8:14], np.zeros(6, np.uint8)):
        with pytest.raises(ValueError):
            api.check_block_starts_out(crow, col, bad, 6)
