"""CPU checks of the CSR gather's host side (no device), following tests/test_apply_abi.py: the two names in their
header (include/mat_inv_32_csr.h), the binding and the library with the declared signatures, and the argument guards,
which answer before a context is touched."""
import ctypes
import os
import re

from conftest import ROOT

from gpu_matrix_inversion_amd import _lib

NEW_SYMBOLS = ("mi32_csr_blocks_device", "mi32_csr_blocks_device_f64")


def test_new_names_in_header_binding_and_library():
    hdr = open(os.path.join(ROOT, "include", "mat_inv_32_csr.h")).read()
    lib = _lib.load()
    for t, sym in zip(("float", "double"), NEW_SYMBOLS):
        assert sym in _lib.CSR_ABI_SYMBOLS and sym not in _lib.C_ABI_SYMBOLS, sym
        fn = getattr(lib, sym)
        assert fn.restype is ctypes.c_int
        assert fn.argtypes == [ctypes.c_void_p] * 4 + [ctypes.c_int] + [ctypes.c_void_p] * 4
        proto = (r"int %s\(mi32_handle_t h, mi32_vbatch_t p, const void \*d_row_ptr, const void \*d_col,\s*"
                 r"int index_bytes,\s*const %s \*d_val, const long long \*d_first, %s \*const \*d_out,\s*"
                 r"const int \*d_ldout\);" % (sym, t, t))
        assert re.search(proto, hdr), sym
    # the header declares these two and nothing else, and stands on the main header
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(re.findall(r"\b(mi32_[a-z0-9_]+)\s*\(", code)) == sorted(NEW_SYMBOLS) == sorted(_lib.CSR_ABI_SYMBOLS)
    assert '#include "mat_inv_32_c.h"' in code
    assert lib.mi32_version() >= 145


def test_guards_answer_without_a_device():
    lib = _lib.load()
    # no entry point reads the context or the plan before its arguments are accepted: zeros stand in for both
    fake_h, fake_p = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(4096)
    h, p = ctypes.cast(fake_h, ctypes.c_void_p), ctypes.cast(fake_p, ctypes.c_void_p)
    # never dereferenced by a refused call
    rp, col, val, first, out = (ctypes.c_void_p(256 * k) for k in range(1, 6))
    for fn in (lib.mi32_csr_blocks_device, lib.mi32_csr_blocks_device_f64):
        assert fn(None, p, rp, col, 4, val, first, out, None) == _lib.MI32_BAD_SHAPE      # null handle
        assert fn(h, None, rp, col, 4, val, first, out, None) == _lib.MI32_BAD_SHAPE      # null plan
        assert fn(h, p, None, col, 4, val, first, out, None) == _lib.MI32_BAD_SHAPE       # null row_ptr
        assert fn(h, p, rp, None, 8, val, first, out, None) == _lib.MI32_BAD_SHAPE        # null col
        assert fn(h, p, rp, col, 8, None, first, out, None) == _lib.MI32_BAD_SHAPE        # null val
        assert fn(h, p, rp, col, 4, val, None, out, None) == _lib.MI32_BAD_SHAPE          # null first
        assert fn(h, p, rp, col, 4, val, first, None, None) == _lib.MI32_BAD_SHAPE        # null out
        for index_bytes in (0, 2, 5, 16, -4):
            assert fn(h, p, rp, col, index_bytes, val, first, out, None) == _lib.MI32_BAD_SHAPE, index_bytes
        # a plan of another device: the device is the first word of both the context and the plan
        ctypes.cast(fake_p, ctypes.POINTER(ctypes.c_int))[0] = 3
        assert fn(h, p, rp, col, 4, val, first, out, None) == _lib.MI32_BAD_SHAPE
        assert fn(h, p, rp, col, 8, val, first, out, None) == _lib.MI32_BAD_SHAPE
        ctypes.cast(fake_p, ctypes.POINTER(ctypes.c_int))[0] = 0
