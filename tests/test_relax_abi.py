"""CPU checks of the relaxation calls' host side (no device), following tests/test_stored_abi.py: the four names in
their header (include/mat_inv_32_relax.h), the binding and the library with the declared signatures, and the argument
guards, which answer before a context or a plan is read."""
import ctypes
import os
import re

from conftest import ROOT

from gpu_matrix_inversion_amd import _lib

VP, I = ctypes.c_void_p, ctypes.c_int
RESIDUAL = ("mi32_csr_block_residual_device", "mi32_csr_block_residual_device_f64")
RELAX = ("mi32_csr_relax_stored_device", "mi32_csr_relax_stored_device_f64")
NEW_SYMBOLS = RESIDUAL + RELAX
CSR = (r"mi32_handle_t h, mi32_vbatch_t p, const void \*d_row_ptr, const void \*d_col,\s*int index_bytes, "
       r"const %s \*d_val, const long long \*d_first,\s*")


def test_new_names_in_header_binding_and_library():
    hdr = open(os.path.join(ROOT, "include", "mat_inv_32_relax.h")).read()
    lib = _lib.load()
    protos = {
        RESIDUAL: (r"int %s\(" + CSR + r"const %s \*d_x,\s*const %s \*d_b, %s \*const \*d_r\);",
                   lambda real: [VP] * 4 + [I] + [VP] * 5),
        RELAX: (r"int %s\(" + CSR + r"const void \*d_store,\s*const long long \*d_offset, const int \*d_format, "
                r"const %s \*d_x,\s*const %s \*d_b,\s*%s omega, %s \*d_xnew\);",
                lambda real: [VP] * 4 + [I] + [VP] * 7 + [real, VP]),
    }
    for names, (proto, argtypes) in protos.items():
        for t, real, sym in zip(("float", "double"), (ctypes.c_float, ctypes.c_double), names):
            assert sym in _lib.RELAX_ABI_SYMBOLS
            for other in (_lib.C_ABI_SYMBOLS, _lib.CSR_ABI_SYMBOLS, _lib.CSR_FIND_ABI_SYMBOLS, _lib.STORED_ABI_SYMBOLS):
                assert sym not in other
            fn = getattr(lib, sym)
            assert fn.restype is ctypes.c_int and fn.argtypes == argtypes(real), sym
            assert re.search(proto % ((sym,) + (t,) * (proto.count("%s") - 1)), hdr), sym
    # the header declares these four and nothing else, and stands on the stored-inverse header
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(re.findall(r"\b(mi32_[a-z0-9_]+)\s*\(", code)) == sorted(NEW_SYMBOLS) == sorted(_lib.RELAX_ABI_SYMBOLS)
    assert '#include "mat_inv_32_stored.h"' in code
    assert lib.mi32_version() >= 148


def test_header_carries_the_definition():
    text = " ".join(open(os.path.join(ROOT, "include", "mat_inv_32_relax.h")).read().replace("*", " ").split())
    for phrase in ("IN STORED ORDER", "p_{e mod 8} = fma(val_e, x[col_e], p_{e mod 8})", "q_s = p_s + p_{s xor 4}",
                   "t_s = q_s + q_{s xor 2}", "sum = t_0 + t_1", "r_g = b_g - sum", "fma(omega, z_b[i], x[d_first[b] + i])",
                   "Rows in no block are not written", "MI32_BAD_SHAPE"):
        assert phrase in text, phrase


def test_guards_answer_without_a_device():
    lib = _lib.load()
    # no entry point reads the context or the plan before its arguments are accepted: zeros stand in for both
    fake_h, fake_p = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(4096)
    h, p = ctypes.cast(fake_h, VP), ctypes.cast(fake_p, VP)
    a = [VP(256 * k) for k in range(1, 12)]      # never dereferenced by a refused call
    bad = _lib.MI32_BAD_SHAPE
    goods = {}
    for name in RESIDUAL:
        goods[name] = [h, p, a[0], a[1], 4, a[2], a[3], a[4], a[5], a[6]]
    for name, one in zip(RELAX, (ctypes.c_float(1.0), ctypes.c_double(1.0))):
        goods[name] = [h, p, a[0], a[1], 8, a[2], a[3], a[4], a[5], a[6], a[7], a[8], one, a[9]]
    for name, good in goods.items():
        fn = getattr(lib, name)
        for k, arg in enumerate(good):
            if isinstance(arg, VP):
                args = list(good)
                args[k] = None
                assert fn(*args) == bad, (name, k)
        for index_bytes in (0, 2, 3, 5, 16, -4):
            args = list(good)
            args[4] = index_bytes
            assert fn(*args) == bad, (name, index_bytes)
    # a plan of another device: the device is the first word of both the context and the plan
    ctypes.cast(fake_p, ctypes.POINTER(ctypes.c_int))[0] = 3
    for name, good in goods.items():
        assert getattr(lib, name)(*good) == bad, name
