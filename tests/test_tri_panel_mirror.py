"""CPU proof of the triangular panel step (tests/tri_panel_mirror.c): sub-panels whose steps update only the columns
right of the pivot and keep the multipliers, the recursion that completes the pivot rows left of their pivots with IEEE
divisions, and the finished columns rebuilt from multipliers and normalised pivot rows give the bytes of the oracle's
step-by-step elimination (-0.0 stored as +0.0, as in every digest here), with the same status."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import gate_matrix
from degenerate_cases import canon, exact_families, ones_block, zero_column
from panel_tie_cases import tie_matrix

ORDERS = (16, 17, 40, 64, 100)
WIDTHS = (8, 16, 32)


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tri_panel_mirror.c")
    lib = os.path.join(str(tmp_path_factory.mktemp("tri_panel_mirror")), "libtri_panel_mirror.so")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                           "-o", lib, src, "-lm"])
    dll = ctypes.CDLL(lib)
    dll.tri_panel_inverse.restype = ctypes.c_int
    dll.tri_panel_inverse.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]

    def run(a, w):
        a = np.ascontiguousarray(a, dtype=np.float32)
        n = a.shape[0]
        out = np.empty((n, n), np.float32)
        st = dll.tri_panel_inverse(a.ctypes.data, n, w, out.ctypes.data)
        return out, st

    return run


def inputs(n):
    """{name: matrix}: D_gate, U(0, 100), the exact families (rows whose early multipliers are exactly zero, rows that
    win late, -0.0 entries), exact ties."""
    rng = np.random.default_rng([5, n])
    d = {"gate": gate_matrix(n, 500 + n), "u100": rng.uniform(0, 100, (n, n)).astype(np.float32)}
    for name, (a, _x) in exact_families(n, 40 + n).items():
        d[name] = a
    if n == 100:
        d["ties"] = tie_matrix(n, (1, 2, 3), 77_000 + n)[0]
    return d


def same_as_oracle(oracle, mirror, a, n, w, what):
    want, info = oracle.matrix_inv_32_inplace(a, n, return_info=True)
    got, st = mirror(a, w)
    assert st == info["status"], (what, st, info["status"])
    assert canon(got) == canon(want), what


@pytest.mark.parametrize("n", ORDERS)
def test_bytes_of_the_step_by_step_oracle(oracle, mirror, n):
    cases = inputs(n)
    assert any(np.signbit(a[a == 0]).any() for a in cases.values()), "no -0.0 in the inputs"
    for name, a in cases.items():
        for w in WIDTHS:
            same_as_oracle(oracle, mirror, a, n, w, (name, n, w))


@pytest.mark.parametrize("n", ORDERS)
def test_subnormal_scaling_keeps_the_division_ieee(oracle, mirror, n):
    """gate * 2^-128: entries, pivots and the recursion's dividends are subnormal or close to it."""
    a = (gate_matrix(n, 900 + n).astype(np.float64) * 2.0 ** -128).astype(np.float32)
    assert (np.abs(a[a != 0]) < np.finfo(np.float32).tiny).any()
    for w in WIDTHS:
        same_as_oracle(oracle, mirror, a, n, w, ("subnormal", n, w))


@pytest.mark.parametrize("n", ORDERS)
def test_late_singularity_is_flagged(oracle, mirror, n):
    """Status only: behind a zero pivot the oracle skips exact-zero multipliers where this restatement (like the
    matrix cores) multiplies them through, and 0 * inf differs from nothing at all."""
    for a in (ones_block(n, n // 2, 60 + n), zero_column(n, n - 3, 70 + n)):
        for w in WIDTHS:
            assert mirror(a, w)[1] == oracle.matrix_inv_32_inplace(a, n, return_info=True)[1]["status"] == 2
