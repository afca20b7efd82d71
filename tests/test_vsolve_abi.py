"""CPU checks of the variable-size solve's host side (no device): the three names in the header, the binding and the
library; the dispatch rule as ``mi32_vbatch_solve_launches`` reports it -- the list the device call walks -- against
its restatement in tests/vsolve_cases.py and against ``mi32_resolve_solve`` for single-order batches; and the argument
guards, which answer before a context is touched."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from solve_cases import cap, rows_of
from vsolve_cases import chunks_of, expected_launches

import gpu_matrix_inversion_amd as g
from gpu_matrix_inversion_amd import _lib

NEW_SYMBOLS = ("mi32_solve_device_vbatched", "mi32_solve_device_vbatched_f64", "mi32_vbatch_solve_launches")
IP = ctypes.POINTER(ctypes.c_int)
# nrhs = 1: the eight runs of orders that share one launch
RUNS_K1 = [(1, 7, 8, 0), (8, 15, 16, 0), (16, 31, 32, 0), (32, 63, 64, 0), (64, 80, 0, 40), (81, 96, 0, 48),
           (97, 112, 0, 56), (113, 127, 0, 64)]


def _launches(lib, orders, nrhs, capacity=None):
    """(rc, launches as a list of 6-tuples, count); capacity None: ask for the count first, then for all of them."""
    o = np.ascontiguousarray(orders, np.int32)
    count = ctypes.c_int(-1)
    if capacity is None:
        rc = lib.mi32_vbatch_solve_launches(o.ctypes.data_as(IP), o.size, nrhs, None, 0, ctypes.byref(count))
        if rc != _lib.MI32_OK:
            return rc, [], count.value
        capacity = count.value
    buf = np.full((capacity + 1, 6), -7, np.int32)      # one row more than the capacity: it must stay untouched
    rc = lib.mi32_vbatch_solve_launches(o.ctypes.data_as(IP), o.size, nrhs, buf.ctypes.data_as(IP), capacity,
                                        ctypes.byref(count))
    assert (buf[capacity] == -7).all()
    return rc, [tuple(int(v) for v in row) for row in buf[:min(capacity, max(count.value, 0))]], count.value


def _covers_every_column_once(orders, nrhs, launches):
    srt = sorted(int(n) for n in orders)
    seen = np.zeros((len(srt), nrhs), np.int32)
    for first, count, col0, cols, lanes, rows in launches:
        assert count >= 1 and cols >= 1 and 0 <= first and first + count <= len(srt) and col0 + cols <= nrhs
        seen[first:first + count, col0:col0 + cols] += 1
        for n in srt[first:first + count]:               # the instance holds every member of its range
            assert (lanes == 0) != (rows == 0)
            if lanes:
                assert lanes in (8, 16, 32, 64) and n + cols <= lanes and (lanes == 8 or n + cols > lanes // 2)
            else:
                assert n + cols > 64 and n + cols <= 128 and n <= 2 * rows and rows == rows_of(n)
    assert (seen == 1).all()
    assert launches == sorted(launches, key=lambda l: (l[0], l[2]))


def test_new_names_in_header_binding_and_library():
    hdr = open(os.path.join(ROOT, "include", "mat_inv_32_c.h")).read()
    lib = _lib.load()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
        assert sym in _lib.C_ABI_SYMBOLS, sym
        assert getattr(lib, sym).restype is ctypes.c_int, sym
    for t, sym in (("float", "mi32_solve_device_vbatched"), ("double", "mi32_solve_device_vbatched_f64")):
        proto = (r"int %s\(mi32_handle_t h, mi32_vbatch_t p, const %s \*const \*d_a, const int \*d_lda,\s*"
                 r"const %s \*const \*d_b, const int \*d_ldb, int nrhs,\s*%s \*const \*d_x,\s*const int \*d_ldx,\s*"
                 r"int \*d_status\);" % (sym, t, t, t))
        assert re.search(proto, hdr), sym
        assert len(getattr(lib, sym).argtypes) == 10
    assert re.search(r"int mi32_vbatch_solve_launches\(const int \*orders, int batch, int nrhs, int \*launches, "
                     r"int capacity,\s*int \*count\);", hdr)
    assert len(lib.mi32_vbatch_solve_launches.argtypes) == 6
    assert lib.mi32_version() >= 142
    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert sig(g.Inverter.solve_pointers) == ["self", "plan", "a_ptrs", "b_ptrs", "x_ptrs", "dtype", "nrhs", "lda", "ldb",
                                              "ldx", "status"]
    assert sig(g.Inverter.solve_ragged) == ["self", "plan", "a_flat", "b", "out", "status"]
    assert sig(g.Inverter.solve_diag_blocks) == ["self", "m", "block_orders", "r", "out"]
    assert sig(g.Inverter.resolved_solve_ragged) == ["self", "orders", "nrhs"]


def test_the_restatement_itself():
    """The Python rule at a few shapes worked out by hand, so that the comparisons below compare against something."""
    assert chunks_of(126, 3) == [(0, 2, 0, 64), (2, 1, 0, 64)]
    assert chunks_of(40, 89) == [(0, 88, 0, 40), (88, 1, 64, 0)]
    assert chunks_of(8, 57) == [(0, 56, 64, 0), (56, 1, 16, 0)]
    assert expected_launches([5, 3, 70, 5], 1) == [(0, 3, 0, 1, 8, 0), (3, 1, 0, 1, 0, 40)]
    assert expected_launches([127, 126, 1], 2) == [(0, 1, 0, 2, 8, 0), (1, 1, 0, 2, 0, 64), (2, 1, 0, 1, 0, 64),
                                                   (2, 1, 1, 1, 0, 64)]


@pytest.mark.parametrize("nrhs", [1, 3, 32, 200])
def test_every_order_once(nrhs):
    lib = _lib.load()
    orders = np.random.default_rng(5).permutation(np.arange(1, 128))
    rc, got, count = _launches(lib, orders, nrhs)
    want = expected_launches(orders, nrhs)
    assert rc == _lib.MI32_OK and count == len(want) and got == want, (nrhs, got[:12], want[:12])
    _covers_every_column_once(orders, nrhs, got)
    if nrhs == 1:
        # (sorted, order n sits at n - 1)
        assert got == [(lo - 1, hi - lo + 1, 0, 1, lanes, rows) for lo, hi, lanes, rows in RUNS_K1]
    if nrhs == 3:
        # 126 and 127 are chunked and take launches of their own; 125 still shares the last run's single launch
        assert got[-5:] == [(125, 1, 0, 2, 0, 64), (125, 1, 2, 1, 0, 64),
                            (126, 1, 0, 1, 0, 64), (126, 1, 1, 1, 0, 64), (126, 1, 2, 1, 0, 64)]
        assert len(got) == 8 + 5


def test_members_of_one_order_share_their_launches():
    lib = _lib.load()
    orders = [5] * 7 + [127] * 3 + [64] * 2 + [5] * 2
    rc, got, count = _launches(lib, orders, 2)
    assert rc == _lib.MI32_OK and got == expected_launches(orders, 2)
    assert got == [(0, 9, 0, 2, 8, 0), (9, 2, 0, 2, 0, 40), (11, 3, 0, 1, 0, 64), (11, 3, 1, 1, 0, 64)]
    _covers_every_column_once(orders, 2, got)


@pytest.mark.parametrize("n", [8, 32, 33, 64, 127])
def test_single_order_batches_agree_with_the_uniform_rule(n):
    lib = _lib.load()
    for nrhs in (1, cap(n), cap(n) + 1):
        rc, got, count = _launches(lib, [n] * 5, nrhs)
        assert rc == _lib.MI32_OK and got == expected_launches([n] * 5, nrhs) == [(0, 5) + c for c in chunks_of(n, nrhs)]
        out = [ctypes.c_int(-1) for _ in range(4)]
        assert lib.mi32_resolve_solve(None, n, nrhs, 4, *(ctypes.byref(o) for o in out)) == _lib.MI32_OK
        cols, launches, lanes, rows = (o.value for o in out)
        assert count == launches and got[0][3] == min(cols, nrhs) and got[0][4:] == (lanes, rows), (n, nrhs)
        assert all(l[2] == i * cols for i, l in enumerate(got))
        _covers_every_column_once([n] * 5, nrhs, got)


def test_capacity():
    lib = _lib.load()
    orders = np.random.default_rng(5).permutation(np.arange(1, 128))
    want = expected_launches(orders, 3)
    rc, got, count = _launches(lib, orders, 3, capacity=0)
    assert rc == _lib.MI32_OK and got == [] and count == len(want)
    rc, got, count = _launches(lib, orders, 3, capacity=4)
    assert rc == _lib.MI32_OK and got == want[:4] and count == len(want)
    rc, got, count = _launches(lib, orders, 3, capacity=len(want) + 9)
    assert rc == _lib.MI32_OK and got == want and count == len(want)


def test_bad_shapes_of_the_launch_list():
    lib = _lib.load()
    for orders in ([4, 0, 4], [4, 128], [129], [-3]):
        assert _launches(lib, orders, 1)[0] == _lib.MI32_BAD_SHAPE, orders
    assert _launches(lib, [4, 5], 0)[0] == _lib.MI32_BAD_SHAPE
    assert _launches(lib, [4, 5], -1)[0] == _lib.MI32_BAD_SHAPE
    o = np.array([4, 5], np.int32)
    buf = np.zeros(60, np.int32)
    count = ctypes.c_int()
    op, bp, cp = o.ctypes.data_as(IP), buf.ctypes.data_as(IP), ctypes.byref(count)
    assert lib.mi32_vbatch_solve_launches(None, 2, 1, bp, 10, cp) == _lib.MI32_BAD_SHAPE     # null orders
    assert lib.mi32_vbatch_solve_launches(op, 2, 1, None, 10, cp) == _lib.MI32_BAD_SHAPE     # null list, capacity > 0
    assert lib.mi32_vbatch_solve_launches(op, 2, 1, bp, 10, None) == _lib.MI32_BAD_SHAPE     # null count
    assert lib.mi32_vbatch_solve_launches(op, 0, 1, bp, 10, cp) == _lib.MI32_BAD_SHAPE       # batch = 0
    assert lib.mi32_vbatch_solve_launches(op, 2, 1, bp, -1, cp) == _lib.MI32_BAD_SHAPE       # capacity < 0
    assert lib.mi32_vbatch_solve_launches(op, 2, 1, bp, 10, cp) == _lib.MI32_OK and count.value == 1


def test_guards_answer_without_a_device():
    lib = _lib.load()
    # no entry point reads the context or the plan before its arguments are accepted: zeros stand in for both
    fake_h, fake_p = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(4096)
    h, p = ctypes.cast(fake_h, ctypes.c_void_p), ctypes.cast(fake_p, ctypes.c_void_p)
    a, b, x = ctypes.c_void_p(256), ctypes.c_void_p(512), ctypes.c_void_p(768)   # never dereferenced by a refused call
    for fn in (lib.mi32_solve_device_vbatched, lib.mi32_solve_device_vbatched_f64):
        assert fn(None, p, a, None, b, None, 1, x, None, None) == _lib.MI32_BAD_SHAPE      # null handle
        assert fn(h, None, a, None, b, None, 1, x, None, None) == _lib.MI32_BAD_SHAPE      # null plan
        assert fn(h, p, None, None, b, None, 1, x, None, None) == _lib.MI32_BAD_SHAPE      # null A
        assert fn(h, p, a, None, None, None, 1, x, None, None) == _lib.MI32_BAD_SHAPE      # null B
        assert fn(h, p, a, None, b, None, 1, None, None, None) == _lib.MI32_BAD_SHAPE      # null X
        assert fn(h, p, a, None, b, None, 0, x, None, None) == _lib.MI32_BAD_SHAPE         # no right-hand side
        assert fn(h, p, a, None, b, None, -4, x, None, None) == _lib.MI32_BAD_SHAPE
