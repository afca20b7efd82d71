"""CPU checks of the apply call's host side (no device): the three names in the header, the binding and the library; the
launch rule as ``mi32_vbatch_apply_launches`` reports it -- the list the device call walks -- against its restatement in
tests/apply_cases.py; and the argument guards, which answer before a context is touched."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from apply_cases import LANE_TOPS, chunk_cols, expected_launches, lanes_of
from conftest import ROOT

import gpu_matrix_inversion_amd as g
from gpu_matrix_inversion_amd import _lib

NEW_SYMBOLS = ("mi32_apply_device_vbatched", "mi32_apply_device_vbatched_f64", "mi32_vbatch_apply_launches")
IP = ctypes.POINTER(ctypes.c_int)


def _launches(lib, orders, nrhs, elem_bytes=4, capacity=None):
    """(rc, launches as a list of 4-tuples, count); capacity None: ask for the count first, then for all of them."""
    o = np.ascontiguousarray(orders, np.int32)
    count = ctypes.c_int(-1)
    if capacity is None:
        rc = lib.mi32_vbatch_apply_launches(o.ctypes.data_as(IP), o.size, nrhs, elem_bytes, None, 0, ctypes.byref(count))
        if rc != _lib.MI32_OK:
            return rc, [], count.value
        capacity = count.value
    buf = np.full((capacity + 1, 4), -7, np.int32)      # one row more than the capacity: it must stay untouched
    rc = lib.mi32_vbatch_apply_launches(o.ctypes.data_as(IP), o.size, nrhs, elem_bytes, buf.ctypes.data_as(IP), capacity,
                                        ctypes.byref(count))
    assert (buf[capacity] == -7).all()
    return rc, [tuple(int(v) for v in row) for row in buf[:min(capacity, max(count.value, 0))]], count.value


def _covers_every_member_once(orders, launches, elem_bytes):
    srt = sorted(int(n) for n in orders)
    seen = np.zeros(len(srt), np.int32)
    assert len(launches) <= 5
    for first, count, lanes, cols in launches:
        assert count >= 1 and 0 <= first and first + count <= len(srt)
        assert lanes in LANE_TOPS and cols == chunk_cols(elem_bytes)
        seen[first:first + count] += 1
        for n in srt[first:first + count]:               # the smallest lane class that holds the order
            assert n <= lanes and (lanes == 8 or n > lanes // 2)
    assert (seen == 1).all()
    assert launches == sorted(launches)


def test_new_names_in_header_binding_and_library():
    hdr = open(os.path.join(ROOT, "include", "mat_inv_32_c.h")).read()
    lib = _lib.load()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
        assert sym in _lib.C_ABI_SYMBOLS, sym
        assert getattr(lib, sym).restype is ctypes.c_int, sym
    for t, sym in (("float", "mi32_apply_device_vbatched"), ("double", "mi32_apply_device_vbatched_f64")):
        proto = (r"int %s\(mi32_handle_t h, mi32_vbatch_t p, const %s \*const \*d_x, const int \*d_ldx,\s*"
                 r"const %s \*const \*d_r, const int \*d_ldr, int nrhs,\s*%s \*const \*d_z,\s*const int \*d_ldz\);"
                 % (sym, t, t, t))
        assert re.search(proto, hdr), sym
        assert len(getattr(lib, sym).argtypes) == 9
    assert re.search(r"int mi32_vbatch_apply_launches\(const int \*orders, int batch, int nrhs, int elem_bytes, "
                     r"int \*launches, int capacity,\s*int \*count\);", hdr)
    assert len(lib.mi32_vbatch_apply_launches.argtypes) == 7
    assert lib.mi32_version() >= 143
    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert sig(g.Inverter.apply_pointers) == ["self", "plan", "x_ptrs", "r_ptrs", "z_ptrs", "dtype", "nrhs", "ldx", "ldr",
                                              "ldz"]
    assert sig(g.Inverter.apply_ragged) == ["self", "plan", "x_flat", "r", "out"]
    assert sig(g.Inverter.apply_diag_blocks) == ["self", "x", "block_orders", "r", "out"]
    assert sig(g.Inverter.resolved_apply_ragged) == ["self", "orders", "nrhs", "elem_bytes"]
    assert inspect.signature(g.Inverter.inv_diag_blocks).parameters["packed"].default is False


def test_the_restatement_itself():
    """The Python rule at a few shapes worked out by hand, so that the comparisons below compare against something."""
    assert [lanes_of(n) for n in (1, 8, 9, 16, 17, 32, 33, 64, 65, 128)] == [8, 8, 16, 16, 32, 32, 64, 64, 128, 128]
    assert expected_launches([5, 3, 70, 5], 1) == [(0, 3, 8, 8), (3, 1, 128, 8)]
    assert expected_launches([128, 9, 64, 65, 1], 7, 8) == [(0, 1, 8, 4), (1, 1, 16, 4), (2, 1, 64, 4), (3, 2, 128, 4)]


@pytest.mark.parametrize("elem_bytes", [4, 8])
@pytest.mark.parametrize("nrhs", [1, 3, 200])
def test_every_order_once(nrhs, elem_bytes):
    lib = _lib.load()
    orders = np.random.default_rng(5).permutation(np.arange(1, 129))
    rc, got, count = _launches(lib, orders, nrhs, elem_bytes)
    want = expected_launches(orders, nrhs, elem_bytes)
    assert rc == _lib.MI32_OK and count == len(want) == 5 and got == want, (nrhs, got, want)
    _covers_every_member_once(orders, got, elem_bytes)
    kc = chunk_cols(elem_bytes)
    # (sorted, order n sits at n - 1) -- and the list does not depend on nrhs: the columns are walked inside the kernel
    assert got == [(0, 8, 8, kc), (8, 8, 16, kc), (16, 16, 32, kc), (32, 32, 64, kc), (64, 64, 128, kc)]


@pytest.mark.parametrize("n", [1, 8, 9, 16, 17, 32, 33, 64, 65, 80, 81, 112, 113, 128])
def test_single_class_batches(n):
    lib = _lib.load()
    for nrhs in (1, 9):
        rc, got, count = _launches(lib, [n] * 5, nrhs)
        assert rc == _lib.MI32_OK and count == 1 and got == [(0, 5, lanes_of(n), 8)] == expected_launches([n] * 5, nrhs)
        _covers_every_member_once([n] * 5, got, 4)


def test_mixed_batches_and_capacity():
    lib = _lib.load()
    orders = [5] * 7 + [127] * 3 + [64] * 2 + [5] * 2 + [70]
    rc, got, count = _launches(lib, orders, 2)
    assert rc == _lib.MI32_OK and got == expected_launches(orders, 2) == [(0, 9, 8, 8), (9, 2, 64, 8), (11, 4, 128, 8)]
    _covers_every_member_once(orders, got, 4)
    rc, part, count = _launches(lib, orders, 2, capacity=0)
    assert rc == _lib.MI32_OK and part == [] and count == 3
    rc, part, count = _launches(lib, orders, 2, capacity=2)
    assert rc == _lib.MI32_OK and part == got[:2] and count == 3
    rc, part, count = _launches(lib, orders, 2, capacity=12)
    assert rc == _lib.MI32_OK and part == got and count == 3


def test_bad_shapes_of_the_launch_list():
    lib = _lib.load()
    for orders in ([4, 0, 4], [4, 129], [-3]):
        assert _launches(lib, orders, 1)[0] == _lib.MI32_BAD_SHAPE, orders
    assert _launches(lib, [4, 128], 1)[0] == _lib.MI32_OK           # order 128 is in
    for nrhs in (0, -1):
        assert _launches(lib, [4, 5], nrhs)[0] == _lib.MI32_BAD_SHAPE
    for elem_bytes in (0, 2, 16):
        assert _launches(lib, [4, 5], 1, elem_bytes)[0] == _lib.MI32_BAD_SHAPE
    o = np.array([4, 5], np.int32)
    buf = np.zeros(40, np.int32)
    count = ctypes.c_int()
    op, bp, cp = o.ctypes.data_as(IP), buf.ctypes.data_as(IP), ctypes.byref(count)
    assert lib.mi32_vbatch_apply_launches(None, 2, 1, 4, bp, 10, cp) == _lib.MI32_BAD_SHAPE     # null orders
    assert lib.mi32_vbatch_apply_launches(op, 2, 1, 4, None, 10, cp) == _lib.MI32_BAD_SHAPE     # null list, capacity > 0
    assert lib.mi32_vbatch_apply_launches(op, 2, 1, 4, bp, 10, None) == _lib.MI32_BAD_SHAPE     # null count
    assert lib.mi32_vbatch_apply_launches(op, 0, 1, 4, bp, 10, cp) == _lib.MI32_BAD_SHAPE       # batch = 0
    assert lib.mi32_vbatch_apply_launches(op, 2, 1, 4, bp, -1, cp) == _lib.MI32_BAD_SHAPE       # capacity < 0
    assert lib.mi32_vbatch_apply_launches(op, 2, 1, 4, bp, 10, cp) == _lib.MI32_OK and count.value == 1


def test_guards_answer_without_a_device():
    lib = _lib.load()
    # no entry point reads the context or the plan before its arguments are accepted: zeros stand in for both
    fake_h, fake_p = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(4096)
    h, p = ctypes.cast(fake_h, ctypes.c_void_p), ctypes.cast(fake_p, ctypes.c_void_p)
    x, r, z = ctypes.c_void_p(256), ctypes.c_void_p(512), ctypes.c_void_p(768)   # never dereferenced by a refused call
    for fn in (lib.mi32_apply_device_vbatched, lib.mi32_apply_device_vbatched_f64):
        assert fn(None, p, x, None, r, None, 1, z, None) == _lib.MI32_BAD_SHAPE      # null handle
        assert fn(h, None, x, None, r, None, 1, z, None) == _lib.MI32_BAD_SHAPE      # null plan
        assert fn(h, p, None, None, r, None, 1, z, None) == _lib.MI32_BAD_SHAPE      # null X
        assert fn(h, p, x, None, None, None, 1, z, None) == _lib.MI32_BAD_SHAPE      # null R
        assert fn(h, p, x, None, r, None, 1, None, None) == _lib.MI32_BAD_SHAPE      # null Z
        assert fn(h, p, x, None, r, None, 0, z, None) == _lib.MI32_BAD_SHAPE         # no column
        assert fn(h, p, x, None, r, None, -4, z, None) == _lib.MI32_BAD_SHAPE
