"""CPU checks of the register-resident path's host side (no device): the enum value and its names, the
introspection entry point, AUTO untouched, and a workspace that holds no per-matrix working copy."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

import gpu_matrix_inversion_amd as g
from gpu_matrix_inversion_amd import _lib


def test_enum_value_and_names():
    hdr = open(os.path.join(ROOT, "include", "mat_inv_32_c.h")).read()
    assert re.search(r"\bMI32_ALGO_RESIDENT\s*=\s*3\b", hdr)
    assert _lib.ALGO_RESIDENT == 3 and g.ALGO_RESIDENT == 3
    assert _lib.ALGO_NAMES["resident"] == 3
    assert _lib.load().mi32_dominant_kernel(3) == b"gj_resident_kernel"


def _resolve(n, elem_bytes):
    lanes, top = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = _lib.load().mi32_resolve_resident(None, n, elem_bytes, ctypes.byref(lanes), ctypes.byref(top))
    return rc, lanes.value, top.value


@pytest.mark.parametrize("elem_bytes", [4, 8])
def test_resolve_resident(elem_bytes):
    for n in range(1, 66):
        want = 8 if n <= 8 else 16 if n <= 16 else 32 if n <= 32 else 64 if n <= 64 else 0
        assert _resolve(n, elem_bytes) == (_lib.MI32_OK, want, 64), n
    assert _resolve(0, elem_bytes)[0] == _lib.MI32_BAD_SHAPE
    assert _resolve(-3, elem_bytes)[0] == _lib.MI32_BAD_SHAPE
    assert _resolve(8, 2)[0] == _lib.MI32_BAD_SHAPE
    # the output pointers are optional
    assert _lib.load().mi32_resolve_resident(None, 8, elem_bytes, None, None) == _lib.MI32_OK


def test_auto_is_unchanged(monkeypatch):
    monkeypatch.delenv("MI32_ALGO", raising=False)
    lib = _lib.load()
    for n in (1, 8, 31):
        assert lib.mi32_resolve_algo(None, n, 1) == _lib.ALGO_SWEEP
    for n in (32, 64, 4096):
        assert lib.mi32_resolve_algo(None, n, 1) == _lib.ALGO_BLOCKED


def test_environment_selects_it_on_the_default_context(monkeypatch):
    lib = _lib.load()
    monkeypatch.setenv("MI32_ALGO", "3")
    for n in (1, 8, 31, 32, 64):
        assert lib.mi32_resolve_algo(None, n, 1) == _lib.ALGO_RESIDENT
    # above 64 rows: what AUTO resolves to
    assert lib.mi32_resolve_algo(None, 65, 1) == _lib.ALGO_BLOCKED
    assert lib.mi32_resolve_algo(None, 4096, 1) == _lib.ALGO_BLOCKED


@pytest.mark.parametrize("n,batch", [(8, 100_000), (64, 100_000)])
def test_workspace_holds_no_working_copy(n, batch, monkeypatch):
    monkeypatch.delenv("MI32_ALGO", raising=False)
    lib = _lib.load()
    residual_share = ((2 * n + 2) * 8 * batch + 255) // 256 * 256
    assert lib.mi32_workspace_bytes(n, batch, _lib.ALGO_RESIDENT) <= residual_share
    assert lib.mi32_workspace_bytes(n, batch, _lib.ALGO_AUTO) > residual_share   # the paths it stands beside


def test_workspace_of_the_fallback(monkeypatch):
    monkeypatch.delenv("MI32_ALGO", raising=False)
    lib = _lib.load()
    assert lib.mi32_workspace_bytes(65, 1, _lib.ALGO_RESIDENT) == lib.mi32_workspace_bytes(65, 1, _lib.ALGO_AUTO)
