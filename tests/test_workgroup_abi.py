"""CPU checks of the workgroup-resident path's host side (no device): the enum value and its names, the
introspection entry point, how MI32_ALGO=4 resolves on both sides of its range, AUTO untouched, and a workspace
that holds no per-matrix working copy."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

import gpu_matrix_inversion_amd as g
from gpu_matrix_inversion_amd import _lib


def test_enum_value_and_names():
    hdr = open(os.path.join(ROOT, "include", "mat_inv_32_c.h")).read()
    assert re.search(r"\bMI32_ALGO_WORKGROUP\s*=\s*4\b", hdr)
    assert _lib.ALGO_WORKGROUP == 4 and g.ALGO_WORKGROUP == 4
    assert _lib.ALGO_NAMES["workgroup"] == 4
    assert _lib.load().mi32_dominant_kernel(4) == b"gj_workgroup_kernel"
    assert "mi32_resolve_workgroup" in _lib.C_ABI_SYMBOLS


def _resolve(n, elem_bytes):
    threads, rows, top = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = _lib.load().mi32_resolve_workgroup(None, n, elem_bytes, ctypes.byref(threads), ctypes.byref(rows),
                                            ctypes.byref(top))
    return rc, threads.value, rows.value, top.value


@pytest.mark.parametrize("elem_bytes", [4, 8])
def test_resolve_workgroup(elem_bytes):
    for n in range(1, 131):
        if 65 <= n <= 128:
            rows = 40 if n <= 80 else 48 if n <= 96 else 56 if n <= 112 else 64
            want = (256, rows)
        else:
            want = (0, 0)
        assert _resolve(n, elem_bytes) == (_lib.MI32_OK,) + want + (128,), n
    assert _resolve(0, elem_bytes)[0] == _lib.MI32_BAD_SHAPE
    assert _resolve(-3, elem_bytes)[0] == _lib.MI32_BAD_SHAPE
    assert _resolve(100, 2)[0] == _lib.MI32_BAD_SHAPE
    assert _resolve(100, 16)[0] == _lib.MI32_BAD_SHAPE
    # the output pointers are optional
    assert _lib.load().mi32_resolve_workgroup(None, 100, elem_bytes, None, None, None) == _lib.MI32_OK


def test_environment_selects_it_on_the_default_context(monkeypatch):
    lib = _lib.load()
    monkeypatch.delenv("MI32_ALGO", raising=False)
    auto = {n: lib.mi32_resolve_algo(None, n, 1) for n in (129, 4096)}
    monkeypatch.setenv("MI32_ALGO", "4")
    got = [lib.mi32_resolve_algo(None, n, 1) for n in (1, 64, 65, 128, 129, 4096)]
    assert got == [_lib.ALGO_RESIDENT, _lib.ALGO_RESIDENT, _lib.ALGO_WORKGROUP, _lib.ALGO_WORKGROUP, auto[129],
                   auto[4096]]
    assert auto[129] == auto[4096] == _lib.ALGO_BLOCKED


def test_auto_is_unchanged(monkeypatch):
    monkeypatch.delenv("MI32_ALGO", raising=False)
    lib = _lib.load()
    for n in (1, 8, 31):
        assert lib.mi32_resolve_algo(None, n, 1) == _lib.ALGO_SWEEP
    for n in (32, 64, 65, 100, 128, 129, 4096):
        assert lib.mi32_resolve_algo(None, n, 1) == _lib.ALGO_BLOCKED
    # and so is RESIDENT above its range
    monkeypatch.setenv("MI32_ALGO", "3")
    for n in (65, 100, 128):
        assert lib.mi32_resolve_algo(None, n, 1) == _lib.ALGO_BLOCKED


@pytest.mark.parametrize("n,batch", [(65, 100_000), (128, 100_000)])
def test_workspace_holds_no_working_copy(n, batch, monkeypatch):
    monkeypatch.delenv("MI32_ALGO", raising=False)
    lib = _lib.load()
    residual_share = ((2 * n + 2) * 8 * batch + 255) // 256 * 256
    assert lib.mi32_workspace_bytes(n, batch, _lib.ALGO_WORKGROUP) <= residual_share
    assert lib.mi32_workspace_bytes(n, batch, _lib.ALGO_AUTO) > residual_share   # the path it stands beside


def test_workspace_of_the_fallback(monkeypatch):
    monkeypatch.delenv("MI32_ALGO", raising=False)
    lib = _lib.load()
    for batch in (1, 64):
        assert lib.mi32_workspace_bytes(129, batch, _lib.ALGO_WORKGROUP) == lib.mi32_workspace_bytes(129, batch, _lib.ALGO_AUTO)
    # below its range it is the register-resident path's
    assert lib.mi32_workspace_bytes(40, 1000, _lib.ALGO_WORKGROUP) == lib.mi32_workspace_bytes(40, 1000, _lib.ALGO_RESIDENT)
