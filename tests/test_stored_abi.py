"""CPU checks of the stored-inverse calls' host side (no device), following tests/test_csr_blocks_abi.py: the six names
in their header (include/mat_inv_32_stored.h), the binding and the library with the declared signatures, and the
argument guards, which answer before a context or a plan is read."""
import ctypes
import os
import re

from conftest import ROOT

from gpu_matrix_inversion_amd import _lib

VP, I = ctypes.c_void_p, ctypes.c_int
STATS = ("mi32_block_stats_device", "mi32_block_stats_device_f64")
STORE = ("mi32_store_inverses_device", "mi32_store_inverses_device_f64")
APPLY = ("mi32_apply_stored_device", "mi32_apply_stored_device_f64")
NEW_SYMBOLS = STATS + STORE + APPLY


def test_new_names_in_header_binding_and_library():
    hdr = open(os.path.join(ROOT, "include", "mat_inv_32_stored.h")).read()
    lib = _lib.load()
    protos = {
        STATS: (r"int %s\(mi32_handle_t h, mi32_vbatch_t p, const %s \*const \*d_a, const int \*d_lda,\s*"
                r"double \*d_stats\);", [VP] * 5),
        STORE: (r"int %s\(mi32_handle_t h, mi32_vbatch_t p, const %s \*const \*d_x, const int \*d_ldx,\s*"
                r"const int \*d_format, const long long \*d_offset, void \*d_store\);", [VP] * 7),
        APPLY: (r"int %s\(mi32_handle_t h, mi32_vbatch_t p, const void \*d_store, const long long \*d_offset,\s*"
                r"const int \*d_format, const %s \*const \*d_r, const int \*d_ldr, int nrhs,\s*"
                r"%s \*const \*d_z, const int \*d_ldz\);", [VP] * 7 + [I] + [VP] * 2),
    }
    for names, (proto, argtypes) in protos.items():
        for t, sym in zip(("float", "double"), names):
            assert sym in _lib.STORED_ABI_SYMBOLS and sym not in _lib.C_ABI_SYMBOLS and sym not in _lib.CSR_ABI_SYMBOLS
            fn = getattr(lib, sym)
            assert fn.restype is ctypes.c_int and fn.argtypes == argtypes, sym
            assert re.search(proto % ((sym,) + (t,) * (proto.count("%s") - 1)), hdr), sym
    # the header declares these six and nothing else, and stands on the main header
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(re.findall(r"\b(mi32_[a-z0-9_]+)\s*\(", code)) == sorted(NEW_SYMBOLS) == sorted(_lib.STORED_ABI_SYMBOLS)
    assert '#include "mat_inv_32_c.h"' in code
    assert lib.mi32_version() >= 146


def test_guards_answer_without_a_device():
    lib = _lib.load()
    # no entry point reads the context or the plan before its arguments are accepted: zeros stand in for both
    fake_h, fake_p = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(4096)
    h, p = ctypes.cast(fake_h, VP), ctypes.cast(fake_p, VP)
    a, b, c, d, e = (VP(256 * k) for k in range(1, 6))      # never dereferenced by a refused call
    bad = _lib.MI32_BAD_SHAPE
    for name in STATS:
        fn = getattr(lib, name)
        for args in ((None, p, a, None, b), (h, None, a, None, b), (h, p, None, None, b), (h, p, a, c, None)):
            assert fn(*args) == bad, (name, args)
    for name in STORE:
        fn = getattr(lib, name)
        good = [h, p, a, None, b, c, d]
        for k in (0, 1, 2, 4, 5, 6):
            args = list(good)
            args[k] = None
            assert fn(*args) == bad, (name, k)
    for name in APPLY:
        fn = getattr(lib, name)
        good = [h, p, a, b, c, d, None, 1, e, None]
        for k in (0, 1, 2, 3, 4, 5, 8):
            args = list(good)
            args[k] = None
            assert fn(*args) == bad, (name, k)
        for nrhs in (0, -1, -(2 ** 31)):
            args = list(good)
            args[7] = nrhs
            assert fn(*args) == bad, (name, nrhs)
    # a plan of another device: the device is the first word of both the context and the plan
    ctypes.cast(fake_p, ctypes.POINTER(ctypes.c_int))[0] = 3
    for name in STATS:
        assert getattr(lib, name)(h, p, a, None, b) == bad
    for name in STORE:
        assert getattr(lib, name)(h, p, a, None, b, c, d) == bad
    for name in APPLY:
        assert getattr(lib, name)(h, p, a, b, c, d, None, 1, e, None) == bad
