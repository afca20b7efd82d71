"""CPU checks of the determinant entry points' host side (no device): the four names in the header, the binding and the
library, the Python surface, and the argument guards, which answer before a context is touched."""
import ctypes
import inspect
import os
import re

from conftest import ROOT

import gpu_matrix_inversion_amd as g
from gpu_matrix_inversion_amd import _lib

NEW_SYMBOLS = ("mi32_inv_det_device", "mi32_inv_det_device_f64", "mi32_inv_det_device_vbatched",
               "mi32_inv_det_device_vbatched_f64")


def test_new_names_in_header_binding_and_library():
    hdr = open(os.path.join(ROOT, "include", "mat_inv_32_c.h")).read()
    lib = _lib.load()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
        assert sym in _lib.C_ABI_SYMBOLS, sym
        fn = getattr(lib, sym)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == (9 if "vbatched" in sym else 8), sym
    assert "(m, k) = frexp(m * pm)" in hdr                         # the pair's definition is in the header
    assert lib.mi32_version() >= 140
    for name in ("slogdet_from_frexp", "det_from_frexp"):
        assert callable(getattr(g, name)) and name in g.__all__
    assert callable(g.Inverter.inv_det)
    for name in ("inv_pointers", "inv_ragged", "inv_diag_blocks"):
        p = inspect.signature(getattr(g.Inverter, name)).parameters["det"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False, name


def test_guards_answer_without_a_device():
    lib = _lib.load()
    # no entry point reads the context before its arguments are accepted: a block of zeros stands in for one
    fake = ctypes.create_string_buffer(4096)
    h = ctypes.cast(fake, ctypes.c_void_p)
    one = ctypes.c_void_p(256)    # stands in for a device pointer: never dereferenced by a refused call
    two = ctypes.c_void_p(512)
    for fn in (lib.mi32_inv_det_device, lib.mi32_inv_det_device_f64):
        assert fn(None, one, 8, 4, two, None, one, one) == _lib.MI32_BAD_SHAPE          # null handle
        assert fn(h, one, 8, 4, two, None, None, one) == _lib.MI32_BAD_SHAPE            # null det_mant
        assert fn(h, one, 8, 4, two, None, one, None) == _lib.MI32_BAD_SHAPE            # null det_exp
        assert fn(h, one, 129, 4, two, None, one, one) == _lib.MI32_BAD_SHAPE           # n > 128
        assert fn(h, one, 0, 4, two, None, one, one) == _lib.MI32_BAD_SHAPE
        assert fn(h, one, 8, 0, two, None, one, one) == _lib.MI32_BAD_SHAPE             # batch = 0
        assert fn(h, one, 8, -3, two, None, one, one) == _lib.MI32_BAD_SHAPE
        assert fn(h, None, 8, 4, two, None, one, one) == _lib.MI32_BAD_SHAPE            # null input
        assert fn(h, one, 8, 4, one, None, one, one) == _lib.MI32_BAD_SHAPE             # the inverse over the input
    for fn in (lib.mi32_inv_det_device_vbatched, lib.mi32_inv_det_device_vbatched_f64):
        assert fn(None, None, None, None, None, None, None, None, None) == _lib.MI32_BAD_SHAPE
        assert fn(None, h, one, None, two, None, None, one, one) == _lib.MI32_BAD_SHAPE  # null handle
        assert fn(h, None, one, None, two, None, None, one, one) == _lib.MI32_BAD_SHAPE  # null plan
        assert fn(h, h, one, None, two, None, None, None, one) == _lib.MI32_BAD_SHAPE    # null det_mant
        assert fn(h, h, one, None, two, None, None, one, None) == _lib.MI32_BAD_SHAPE    # null det_exp
        assert fn(h, h, None, None, two, None, None, one, one) == _lib.MI32_BAD_SHAPE    # null member pointers
