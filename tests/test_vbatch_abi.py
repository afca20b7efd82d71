"""CPU checks of the variable-size batch's host side (no device): the new names in the header, the binding and the
library, and the binning every launch depends on -- the stable sort by order and the eight class ranges."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from vbatch_cases import CLASS_TOPS, class_begin

import gpu_matrix_inversion_amd as g
from gpu_matrix_inversion_amd import _lib

NEW_SYMBOLS = ("mi32_vbatch_bin", "mi32_vbatch_create", "mi32_vbatch_destroy", "mi32_vbatch_info",
               "mi32_inv_device_vbatched", "mi32_inv_device_vbatched_f64")
IP = ctypes.POINTER(ctypes.c_int)


def test_new_names_in_header_binding_and_library():
    hdr = open(os.path.join(ROOT, "include", "mat_inv_32_c.h")).read()
    lib = _lib.load()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
        assert sym in _lib.C_ABI_SYMBOLS, sym
        assert getattr(lib, sym) is not None
    assert re.search(r"typedef struct mi32_vbatch \*mi32_vbatch_t;", hdr)
    assert "undefined" in hdr[hdr.index("mi32_vbatch_bin"):]       # overlapping members: said in the header
    assert lib.mi32_version() > 120
    assert _lib.VBATCH_CLASS_TOPS == CLASS_TOPS
    for name in ("RaggedPlan", "vbatch_bin"):
        assert hasattr(g, name)
    for name in ("plan_ragged", "inv_ragged", "inv_pointers", "inv_diag_blocks"):
        assert callable(getattr(g.Inverter, name))


def _bin(orders):
    o = np.ascontiguousarray(orders, dtype=np.int32)
    perm = np.full(o.size, -1, np.int32)
    begin = np.full(9, -1, np.int32)
    rc = _lib.load().mi32_vbatch_bin(o.ctypes.data_as(IP), int(o.size), perm.ctypes.data_as(IP), begin.ctypes.data_as(IP))
    return rc, perm, begin


def _check(orders):
    rc, perm, begin = _bin(orders)
    assert rc == _lib.MI32_OK
    assert np.array_equal(perm, np.argsort(np.asarray(orders), kind="stable"))
    assert begin.tolist() == class_begin(orders)
    # the class ranges hold the orders they are for
    srt = np.asarray(orders)[perm]
    lows = (0,) + CLASS_TOPS[:-1]
    for k in range(8):
        part = srt[begin[k]:begin[k + 1]]
        assert ((part > lows[k]) & (part <= CLASS_TOPS[k])).all(), k
    p2, b2 = g.vbatch_bin(orders)
    assert np.array_equal(p2, perm) and np.array_equal(b2, begin)


def test_bin_random_orders():
    orders = np.random.default_rng(77).integers(1, 129, 10_000)
    assert orders.min() == 1 and orders.max() == 128
    _check(orders)


@pytest.mark.parametrize("orders", [[37] * 1000, [1], [128], [64], [65],
                                    [t + d for t in CLASS_TOPS for d in (0, 1) if t + d <= 128] * 3,
                                    list(range(128, 0, -1)), list(range(1, 129)) * 2],
                         ids=["all-equal", "one-1", "one-128", "one-64", "one-65", "boundaries", "descending", "twice"])
def test_bin_special_cases(orders):
    _check(orders)


def test_bin_rejects_bad_arguments():
    lib = _lib.load()
    for bad in ([0], [129], [-4], [5, 0, 5], [5, 129], [5, -1], [2 ** 31 - 1]):
        rc, perm, begin = _bin(bad)
        assert rc == _lib.MI32_BAD_SHAPE, bad
    o = (ctypes.c_int * 4)(3, 4, 5, 6)
    perm = (ctypes.c_int * 4)()
    begin = (ctypes.c_int * 9)()
    assert lib.mi32_vbatch_bin(o, 0, perm, begin) == _lib.MI32_BAD_SHAPE
    assert lib.mi32_vbatch_bin(o, -2, perm, begin) == _lib.MI32_BAD_SHAPE
    assert lib.mi32_vbatch_bin(None, 4, perm, begin) == _lib.MI32_BAD_SHAPE
    assert lib.mi32_vbatch_bin(o, 4, None, begin) == _lib.MI32_BAD_SHAPE
    assert lib.mi32_vbatch_bin(o, 4, perm, None) == _lib.MI32_BAD_SHAPE
    assert lib.mi32_vbatch_bin(o, 4, perm, begin) == _lib.MI32_OK
    with pytest.raises(ValueError):
        g.vbatch_bin([3, 200])


def test_plan_entry_points_answer_their_guards_without_a_device():
    lib = _lib.load()
    o = (ctypes.c_int * 2)(3, 4)
    out = ctypes.c_void_p(1)
    assert lib.mi32_vbatch_create(None, o, 2, ctypes.byref(out)) == _lib.MI32_BAD_SHAPE
    assert out.value is None                                      # no plan comes back from a refused call
    assert lib.mi32_vbatch_create(None, o, 2, None) == _lib.MI32_BAD_SHAPE
    assert lib.mi32_vbatch_destroy(None) == _lib.MI32_OK
    assert lib.mi32_vbatch_info(None, None, None) == _lib.MI32_BAD_SHAPE
    assert lib.mi32_inv_device_vbatched(None, None, None, None, None, None, None) == _lib.MI32_BAD_SHAPE
    assert lib.mi32_inv_device_vbatched_f64(None, None, None, None, None, None, None) == _lib.MI32_BAD_SHAPE
