"""CPU checks of the any-order determinant entry points' host side (no device): the two names in the header, the
binding and the library, the Python surface, and the argument guards, which answer before a context is touched."""
import ctypes
import inspect
import os
import re

from conftest import ROOT

import gpu_matrix_inversion_amd as g
from gpu_matrix_inversion_amd import _lib

NEW_SYMBOLS = ("mi32_inv_det_any_device", "mi32_inv_det_any_device_f64")


def test_new_names_in_header_binding_and_library():
    hdr = open(os.path.join(ROOT, "include", "mat_inv_32_c.h")).read()
    lib = _lib.load()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
        assert sym in _lib.C_ABI_SYMBOLS, sym
        fn = getattr(lib, sym)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 8, sym
    assert lib.mi32_version() >= 144
    # documented next to mi32_inv_det_device, whose limit stays
    assert hdr.index("mi32_inv_det_device(") < hdr.index("mi32_inv_det_any_device(") < hdr.index("mi32_solve_device(")
    sig = inspect.signature(g.Inverter.inv_det_any)
    assert list(sig.parameters) == ["self", "a", "out", "status", "want_inverse"]
    assert sig.parameters["want_inverse"].default is True and sig.parameters["out"].default is None
    # the kernel classes of mi32_get_profile stay: the new launches are accounted to the finish class
    assert len(_lib.KERNEL_CLASSES) == 7


def test_guards_answer_without_a_device():
    lib = _lib.load()
    # no entry point reads the context before its arguments are accepted: a block of zeros stands in for one
    fake = ctypes.create_string_buffer(4096)
    h = ctypes.cast(fake, ctypes.c_void_p)
    one = ctypes.c_void_p(256)    # stands in for a device pointer: never dereferenced by a refused call
    two = ctypes.c_void_p(512)
    for fn in (lib.mi32_inv_det_any_device, lib.mi32_inv_det_any_device_f64):
        for n in (8, 128, 129, 300, 4096, 16384):
            assert fn(None, one, n, 4, two, None, one, one) == _lib.MI32_BAD_SHAPE          # null handle
            assert fn(h, None, n, 4, two, None, one, one) == _lib.MI32_BAD_SHAPE            # null input
            assert fn(h, one, n, 4, two, None, None, one) == _lib.MI32_BAD_SHAPE            # null det_mant
            assert fn(h, one, n, 4, two, None, one, None) == _lib.MI32_BAD_SHAPE            # null det_exp
            assert fn(h, one, n, 0, two, None, one, one) == _lib.MI32_BAD_SHAPE             # batch = 0
            assert fn(h, one, n, -3, two, None, one, one) == _lib.MI32_BAD_SHAPE
            assert fn(h, one, n, 4, one, None, one, one) == _lib.MI32_BAD_SHAPE             # the inverse over the input
        assert fn(h, one, 0, 4, two, None, one, one) == _lib.MI32_BAD_SHAPE                 # n = 0
        assert fn(h, one, -5, 4, two, None, one, one) == _lib.MI32_BAD_SHAPE
        assert fn(h, one, 0, 4, None, None, one, one) == _lib.MI32_BAD_SHAPE                # ... in the determinant-only form
