"""CPU checks of the wide workgroup-resident path's host side (no device): the enum value and its names, the
introspection entry point, how MI32_ALGO=5 resolves on both sides of its range, algorithms 0 ... 4 untouched, a
workspace that holds no per-matrix working copy, and the DenseRoute of the new path."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from wide_cases import MAX_ORDER, wide_class

import gpu_matrix_inversion_amd as g
from gpu_matrix_inversion_amd import _lib

PATH_WIDE = 6   # DenseRoute::Path: appended behind NOPIVOT64 (0 ... 5 are pinned by tests/test_dense_route.py)


def test_enum_value_and_names():
    hdr = open(os.path.join(ROOT, "include", "mat_inv_32_c.h")).read()
    assert re.search(r"\bMI32_ALGO_WIDE\s*=\s*5\b", hdr)
    assert _lib.ALGO_WIDE == 5 and g.ALGO_WIDE == 5
    assert _lib.ALGO_NAMES["wide"] == 5
    assert _lib.load().mi32_dominant_kernel(5) == b"gj_wide_kernel"
    assert "mi32_resolve_wide" in _lib.C_ABI_SYMBOLS
    assert re.search(r"\bint\s+mi32_resolve_wide\s*\(", hdr)


def _resolve(n, elem_bytes):
    threads, rows, top = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = _lib.load().mi32_resolve_wide(None, n, elem_bytes, ctypes.byref(threads), ctypes.byref(rows), ctypes.byref(top))
    return rc, threads.value, rows.value, top.value


@pytest.mark.parametrize("elem_bytes", [4, 8])
def test_resolve_wide(elem_bytes):
    for n in range(1, 259):
        want = wide_class(n) if elem_bytes == 4 else (0, 0)   # no fp64 instance
        assert _resolve(n, elem_bytes) == (_lib.MI32_OK,) + want + (MAX_ORDER,), n
    assert wide_class(129) == (768, 40) and wide_class(192) == (768, 48)
    assert wide_class(193) == (1024, 56) and wide_class(256) == (1024, 64)
    assert _resolve(0, elem_bytes)[0] == _lib.MI32_BAD_SHAPE
    assert _resolve(-3, elem_bytes)[0] == _lib.MI32_BAD_SHAPE
    assert _resolve(200, 2)[0] == _lib.MI32_BAD_SHAPE
    assert _resolve(200, 16)[0] == _lib.MI32_BAD_SHAPE
    # the output pointers are optional
    assert _lib.load().mi32_resolve_wide(None, 200, elem_bytes, None, None, None) == _lib.MI32_OK


def test_environment_selects_it_on_the_default_context(monkeypatch):
    lib = _lib.load()
    monkeypatch.delenv("MI32_ALGO", raising=False)
    auto = {n: lib.mi32_resolve_algo(None, n, 1) for n in (257, 4096)}
    monkeypatch.setenv("MI32_ALGO", "5")
    got = [lib.mi32_resolve_algo(None, n, 1) for n in (1, 64, 65, 128, 129, 256, 257, 4096)]
    assert got == [_lib.ALGO_RESIDENT, _lib.ALGO_RESIDENT, _lib.ALGO_WORKGROUP, _lib.ALGO_WORKGROUP, _lib.ALGO_WIDE,
                   _lib.ALGO_WIDE, auto[257], auto[4096]]
    assert auto[257] == auto[4096] == _lib.ALGO_BLOCKED


def test_algorithms_0_to_4_resolve_unchanged(monkeypatch):
    lib = _lib.load()
    for algo, want in ((0, _lib.ALGO_BLOCKED), (1, _lib.ALGO_SWEEP), (2, _lib.ALGO_BLOCKED), (3, _lib.ALGO_BLOCKED),
                       (4, _lib.ALGO_BLOCKED)):
        monkeypatch.setenv("MI32_ALGO", str(algo))
        for n in (129, 4096):
            assert lib.mi32_resolve_algo(None, n, 1) == want, (algo, n)


@pytest.mark.parametrize("n,batch", [(129, 100_000), (256, 100_000)])
def test_workspace_holds_no_working_copy(n, batch, monkeypatch):
    monkeypatch.delenv("MI32_ALGO", raising=False)
    lib = _lib.load()
    residual_share = ((2 * n + 2) * 8 * batch + 255) // 256 * 256
    assert lib.mi32_workspace_bytes(n, batch, _lib.ALGO_WIDE) <= residual_share
    assert lib.mi32_workspace_bytes(n, batch, _lib.ALGO_AUTO) > residual_share   # the path it stands beside


def test_workspace_of_the_fallback(monkeypatch):
    monkeypatch.delenv("MI32_ALGO", raising=False)
    lib = _lib.load()
    for batch in (1, 64):
        assert lib.mi32_workspace_bytes(257, batch, _lib.ALGO_WIDE) == lib.mi32_workspace_bytes(257, batch, _lib.ALGO_AUTO)
    # below its range it is the other one-launch paths'
    assert lib.mi32_workspace_bytes(40, 1000, _lib.ALGO_WIDE) == lib.mi32_workspace_bytes(40, 1000, _lib.ALGO_RESIDENT)
    assert lib.mi32_workspace_bytes(100, 1000, _lib.ALGO_WIDE) == lib.mi32_workspace_bytes(100, 1000, _lib.ALGO_WORKGROUP)


def _dense_route(n, batch, elem_bytes):
    out = (ctypes.c_int * 5)()
    ws = ctypes.c_size_t()
    fn = _lib.load().mi32_debug_dense_route
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                   ctypes.POINTER(ctypes.c_size_t)]
    assert fn(None, n, batch, elem_bytes, out, ctypes.byref(ws)) == _lib.MI32_OK
    return list(out), ws.value


def test_dense_route_of_the_new_path(monkeypatch):
    monkeypatch.setenv("MI32_ALGO", "5")
    for n in (129, 200, 256):
        route, ws = _dense_route(n, 1000, 4)
        # path, pivot-list entries, first real step, padded order, block width: a one-launch path keeps no list
        assert route == [PATH_WIDE, 0, 0, 0, 0], (n, route)
        assert ws == ((2 * n + 2) * 8 * 1000 + 255) // 256 * 256   # the residual check's share alone
    # an fp64 call above 128 and an fp32 call above 256 plan what AUTO plans
    monkeypatch.setenv("MI32_ALGO", "0")
    auto = [_dense_route(200, 4, 8), _dense_route(257, 4, 4)]
    monkeypatch.setenv("MI32_ALGO", "5")
    assert [_dense_route(200, 4, 8), _dense_route(257, 4, 4)] == auto
    assert auto[0][0][0] != PATH_WIDE and auto[1][0][0] != PATH_WIDE
