"""CPU checks of the solve entry points' host side (no device): the three names in the header, the binding and the
library; the chunk rule and the kernel dispatch as ``mi32_resolve_solve`` reports them, for every order; and the
argument guards, which answer before a context is touched."""
import ctypes
import inspect
import os
import re

import pytest

from conftest import ROOT
from solve_cases import cap, expected_dispatch

import gpu_matrix_inversion_amd as g
from gpu_matrix_inversion_amd import _lib

NEW_SYMBOLS = ("mi32_solve_device", "mi32_solve_device_f64", "mi32_resolve_solve")


def _resolve(lib, n, nrhs, elem_bytes=4):
    out = [ctypes.c_int(-1) for _ in range(4)]
    rc = lib.mi32_resolve_solve(None, n, nrhs, elem_bytes, *(ctypes.byref(o) for o in out))
    return rc, tuple(o.value for o in out)


def test_new_names_in_header_binding_and_library():
    hdr = open(os.path.join(ROOT, "include", "mat_inv_32_c.h")).read()
    lib = _lib.load()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
        assert sym in _lib.C_ABI_SYMBOLS, sym
        fn = getattr(lib, sym)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 8, sym
    for t, sym in (("float", "mi32_solve_device"), ("double", "mi32_solve_device_f64")):
        proto = (r"int %s\(mi32_handle_t h, const %s \*d_a, int n, int batch, const %s \*d_b, int nrhs, %s \*d_x,\s*"
                 r"int \*d_status\);" % (sym, t, t, t))
        assert re.search(proto, hdr), sym
    assert re.search(r"int mi32_resolve_solve\(mi32_handle_t h, int n, int nrhs, int elem_bytes, int \*chunk_cols, "
                     r"int \*launches, int \*lanes,\s*int \*rows_per_thread\);", hdr)
    assert lib.mi32_version() >= 141
    assert list(inspect.signature(g.Inverter.solve).parameters) == ["self", "a", "b", "out", "status"]
    assert list(inspect.signature(g.Inverter.resolved_solve).parameters) == ["self", "n", "nrhs", "elem_bytes"]
    assert inspect.signature(g.Inverter.resolved_solve).parameters["elem_bytes"].default == 4


def test_chunk_rule():
    assert [cap(n) for n in (1, 31, 32, 33, 64, 65, 127)] == [63, 33, 32, 95, 64, 63, 1]


@pytest.mark.parametrize("elem_bytes", [4, 8])
def test_dispatch_of_every_order(elem_bytes):
    lib = _lib.load()
    for n in range(1, 128):
        c = cap(n)
        for nrhs in (1, c, c + 1, 3 * c + 2):
            rc, got = _resolve(lib, n, nrhs, elem_bytes)
            want = expected_dispatch(n, nrhs)
            assert rc == _lib.MI32_OK and got == want, (n, nrhs, got, want)
            cols, launches, lanes, rows = got
            assert cols == (64 - n if n <= 32 else 128 - n)
            assert launches == -(-nrhs // cols)
            width = n + min(nrhs, cols)
            if width <= 64:
                assert lanes in (8, 16, 32, 64) and lanes >= width and (lanes == 8 or lanes // 2 < width) and rows == 0
            else:
                assert lanes == 0 and rows == (40 if n <= 80 else 48 if n <= 96 else 56 if n <= 112 else 64)
    # the lane classes by width, and the move to the workgroup at width 65
    assert [_resolve(lib, n, 1)[1][2:] for n in (7, 8, 15, 16, 31, 32, 63, 64)] == [
        (8, 0), (16, 0), (16, 0), (32, 0), (32, 0), (64, 0), (64, 0), (0, 40)]
    assert [_resolve(lib, n, 1)[1][3] for n in (80, 81, 96, 97, 112, 113, 127)] == [40, 48, 48, 56, 56, 64, 64]
    assert _resolve(lib, 33, 31)[1] == (95, 1, 64, 0) and _resolve(lib, 33, 32)[1] == (95, 1, 0, 40)


def test_bad_shapes_of_the_resolver():
    lib = _lib.load()
    for n in (0, -1, 128, 129):
        assert _resolve(lib, n, 1)[0] == _lib.MI32_BAD_SHAPE, n
    assert _resolve(lib, 8, 0)[0] == _lib.MI32_BAD_SHAPE
    assert _resolve(lib, 8, -2)[0] == _lib.MI32_BAD_SHAPE
    assert _resolve(lib, 8, 1, 2)[0] == _lib.MI32_BAD_SHAPE
    good = [ctypes.c_int() for _ in range(4)]
    for null in range(4):
        args = [None if k == null else ctypes.byref(o) for k, o in enumerate(good)]
        assert lib.mi32_resolve_solve(None, 8, 1, 4, *args) == _lib.MI32_BAD_SHAPE, null


def test_guards_answer_without_a_device():
    lib = _lib.load()
    # no entry point reads the context before its arguments are accepted: a block of zeros stands in for one
    fake = ctypes.create_string_buffer(4096)
    h = ctypes.cast(fake, ctypes.c_void_p)
    a = ctypes.c_void_p(256)    # stand in for device pointers: never dereferenced by a refused call
    b = ctypes.c_void_p(512)
    x = ctypes.c_void_p(768)
    for fn in (lib.mi32_solve_device, lib.mi32_solve_device_f64):
        assert fn(None, a, 8, 4, b, 1, x, None) == _lib.MI32_BAD_SHAPE           # null handle
        assert fn(h, None, 8, 4, b, 1, x, None) == _lib.MI32_BAD_SHAPE           # null A
        assert fn(h, a, 8, 4, None, 1, x, None) == _lib.MI32_BAD_SHAPE           # null B
        assert fn(h, a, 8, 4, b, 1, None, None) == _lib.MI32_BAD_SHAPE           # null X
        assert fn(h, a, 128, 4, b, 1, x, None) == _lib.MI32_BAD_SHAPE            # no spare column
        assert fn(h, a, 129, 4, b, 1, x, None) == _lib.MI32_BAD_SHAPE
        assert fn(h, a, 0, 4, b, 1, x, None) == _lib.MI32_BAD_SHAPE
        assert fn(h, a, 8, 0, b, 1, x, None) == _lib.MI32_BAD_SHAPE              # batch = 0
        assert fn(h, a, 8, 4, b, 0, x, None) == _lib.MI32_BAD_SHAPE              # no right-hand side
        assert fn(h, a, 8, 4, b, -1, x, None) == _lib.MI32_BAD_SHAPE
        assert fn(h, a, 8, 4, b, 1, a, None) == _lib.MI32_BAD_SHAPE              # X over A
