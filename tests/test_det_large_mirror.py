"""CPU checks of the expected values of the determinant tests above order 128 (no device).  tests/det_mirror_large.c
restates two elimination orders with pivot reporting; here both are held to the oracle bit for bit -- inverse, status
and pivot rows -- and mirror (a) to the serial tests/det_mirror.c at the small orders, so neither can drift.  The
(mantissa, exponent) recurrence on the mirror's pivots is held to numpy.linalg.slogdet with the bound of
tests/test_det_mirror.py."""
import math

import numpy as np
import pytest

from det_cases import KINDS, MIRROR_ORDERS, build_mirror, dominant_member, family_members, frexp_det, mirror
from det_large_cases import (MIRROR_A_ORDERS, MIRROR_B_SHAPES, build_mirror_large, mirror_blocked64, mirror_steps,
                             signed_power_diagonal)


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return build_mirror_large(tmp_path_factory.mktemp("det_mirror_large"))


@pytest.fixture(scope="module")
def small_dll(tmp_path_factory):
    return build_mirror(tmp_path_factory.mktemp("det_mirror"))


def pivot_rows(swp_rows, n):
    return swp_rows != np.arange(n)


@pytest.mark.parametrize("n", MIRROR_A_ORDERS)
def test_steps_mirror_equals_the_oracle(oracle, dll, n):
    for kind, a in zip(KINDS, family_members(n)):
        want, info = oracle.matrix_inv_32_inplace(a, n, return_info=True)
        x, st, piv, swp = mirror_steps(dll, a)
        assert st == info["status"] == 0, (n, kind)
        assert np.array_equal(x.reshape(-1), want), (n, kind)
        assert np.array_equal(swp, pivot_rows(info["pivots"], n)), (n, kind)
        a64 = a.astype(np.float64) * 1.000000001  # entries that are no float32 values
        want, info = oracle.matrix_inv_64(a64, n, return_info=True)
        x, st, piv, swp = mirror_steps(dll, a64)
        assert st == info["status"] == 0, (n, kind)
        assert np.array_equal(x.reshape(-1), want), (n, kind)
        assert np.array_equal(swp, pivot_rows(info["pivots"], n)), (n, kind)
    for dtype in (np.float32, np.float64):
        a = dominant_member(n, dtype)
        want, info = oracle.matrix_inversion_no_pivots(a, n, return_info=True)
        x, st, piv, swp = mirror_steps(dll, a, pivoting=False)
        assert st == info["status"] == 0 and not swp.any()
        assert np.array_equal(x.reshape(-1), want), (n, dtype)
        assert np.array_equal(piv[:1], a[0, :1])  # the first pivot is the first diagonal entry


@pytest.mark.parametrize("n", MIRROR_ORDERS)
def test_steps_mirror_equals_the_serial_mirror(dll, small_dll, n):
    for a in family_members(n) + [m.astype(np.float64) * 1.000000001 for m in family_members(n)]:
        x0, st0, piv0, swp0 = mirror(small_dll, a)
        x, st, piv, swp = mirror_steps(dll, a)
        assert st == st0
        assert np.array_equal(piv.view(np.uint8), piv0.view(np.uint8)) and np.array_equal(swp, swp0), n
        assert np.array_equal(x.view(np.uint8), x0.view(np.uint8)), n
    for dtype in (np.float32, np.float64):
        a = dominant_member(n, dtype)
        x0, st0, piv0, swp0 = mirror(small_dll, a, pivoting=False)
        x, st, piv, swp = mirror_steps(dll, a, pivoting=False)
        assert st == st0 and np.array_equal(piv.view(np.uint8), piv0.view(np.uint8)) and not swp.any()


@pytest.mark.parametrize("n,bw", MIRROR_B_SHAPES)
def test_blocked_mirror_equals_the_oracle(oracle, dll, n, bw):
    for kind, a in zip(KINDS, family_members(n, np.float64)):
        a = a * 1.000000001
        want, info = oracle.matrix_inv_64_blocked(a, n, bw, return_info=True)
        x, st, piv, swp = mirror_blocked64(dll, a, bw)
        assert st == info["status"] == 0, (n, bw, kind)
        assert np.array_equal(x.reshape(-1), want), (n, bw, kind)
        assert np.array_equal(swp, pivot_rows(info["pivots"], n)), (n, bw, kind)


@pytest.mark.parametrize("n", MIRROR_A_ORDERS)
def test_recurrence_against_numpy_slogdet(dll, n):
    """The sign is numpy's; |logabsdet - numpy's| <= 1e-4 * max(1, |numpy's|), the bound of tests/test_det_mirror.py."""
    for kind, a in zip(KINDS, family_members(n)):
        x, st, piv, swp = mirror_steps(dll, a)
        m, e = frexp_det(a, piv, swp)
        assert st == 0 and 0.5 <= abs(m) < 1.0
        sign, logabs = np.linalg.slogdet(a.astype(np.float64))
        mine = math.log(abs(m)) + e * math.log(2.0)
        print(f"n {n} {kind}: logabsdet {mine:.9g}, numpy {logabs:.9g}, diff {abs(mine - logabs):.3g}")
        assert math.copysign(1.0, m) == sign, (n, kind)
        assert abs(mine - logabs) <= 1e-4 * max(1.0, abs(logabs)), (n, kind, mine, logabs)
    a = family_members(300, np.float64)[2] * 1.000000001
    for bw in (64, 128):
        x, st, piv, swp = mirror_blocked64(dll, a, bw)
        m, e = frexp_det(a, piv, swp)
        sign, logabs = np.linalg.slogdet(a)
        assert math.copysign(1.0, m) == sign
        assert abs(math.log(abs(m)) + e * math.log(2.0) - logabs) <= 1e-4 * max(1.0, abs(logabs))


def test_closed_form_inputs(dll):
    """P D with D a diagonal of signed powers of two: the mirror's pivots give the closed-form pair."""
    for n, seed in ((129, 1), (300, 2)):
        a, mant, exp = signed_power_diagonal(n, seed)
        x, st, piv, swp = mirror_steps(dll, a)
        assert st == 0 and frexp_det(a, piv, swp) == (float(mant), int(exp)), n
        x, st, piv, swp = mirror_blocked64(dll, a.astype(np.float64), 64)
        assert st == 0 and frexp_det(a, piv, swp) == (float(mant), int(exp)), n
