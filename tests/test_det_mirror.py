"""CPU checks of the determinant tests' own expected values (no device).  tests/det_mirror.c restates the oracle's
step-by-step Gauss-Jordan because the oracle reports no pivot values; here it is held to the oracle bit for bit, so it
cannot drift, and the (mantissa, exponent) recurrence built on its pivots is held to numpy.linalg.slogdet.  The pure
torch helpers ``slogdet_from_frexp`` / ``det_from_frexp`` are checked on CPU tensors."""
import math

import numpy as np
import pytest

from det_cases import (KINDS, MIRROR_ORDERS, build_mirror, dominant_member, family_members, frexp_det, mirror,
                       permutation_matrix, same_doubles)
from resident_cases import TIE_ORDERS, shared_wave_batch, tie_batch

import gpu_matrix_inversion_amd as g


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return build_mirror(tmp_path_factory.mktemp("det_mirror"))


@pytest.mark.parametrize("n", MIRROR_ORDERS)
def test_mirror_equals_the_oracle(oracle, dll, n):
    for a in family_members(n):
        want, info = oracle.matrix_inv_32_inplace(a, n, return_info=True)
        x, st, piv, swp = mirror(dll, a)
        assert st == info["status"] == 0
        assert np.array_equal(x.reshape(-1), want), n
        assert np.array_equal(swp, info["pivots"] != np.arange(n)), n
        a64 = a.astype(np.float64) * 1.000000001  # entries that are no float32 values
        want, info = oracle.matrix_inv_64(a64, n, return_info=True)
        x, st, piv, swp = mirror(dll, a64)
        assert st == info["status"] == 0
        assert np.array_equal(x.reshape(-1), want), n
        assert np.array_equal(swp, info["pivots"] != np.arange(n)), n
    for dtype in (np.float32, np.float64):
        a = dominant_member(n, dtype)
        want, info = oracle.matrix_inversion_no_pivots(a, n, return_info=True)
        x, st, piv, swp = mirror(dll, a, pivoting=False)
        assert st == info["status"] == 0 and not swp.any()
        assert np.array_equal(x.reshape(-1), want), (n, dtype)


@pytest.mark.parametrize("n", TIE_ORDERS)
def test_mirror_equals_the_oracle_on_ties(oracle, dll, n):
    for a in tie_batch(n):
        want, info = oracle.matrix_inv_32_inplace(a, n, return_info=True)
        x, st, piv, swp = mirror(dll, a)
        assert st == info["status"]
        assert np.array_equal(swp, info["pivots"] != np.arange(n))
        if st == 0:
            assert np.array_equal(x.reshape(-1), want)


def test_mirror_flags_what_the_oracle_flags(oracle, dll):
    mats, want_st = shared_wave_batch()
    for a, s in zip(mats, want_st):
        x, st, piv, swp = mirror(dll, a)
        assert st == s == oracle.matrix_inv_32_inplace(a, 20, return_info=True)[1]["status"]
    assert frexp_det(mats[3], *mirror(dll, mats[3])[2:]) == (0.0, 0)            # rank 1: an exactly zero pivot
    assert math.isnan(frexp_det(mats[5], *mirror(dll, mats[5])[2:])[0])        # a NaN entry: never starts
    assert frexp_det(mats[8], *mirror(dll, mats[8])[2:]) == (0.0, 0)            # the zero matrix
    hit = dominant_member(20, np.float32)
    hit[1, 1] = hit[1, 0] = 0.0                                                # stays exactly zero without pivoting
    x, st, piv, swp = mirror(dll, hit, pivoting=False)
    m, e = frexp_det(hit, piv, swp, pivoting=False)
    assert st == 2 and math.isnan(m) and e == 0


@pytest.mark.parametrize("n", MIRROR_ORDERS)
def test_recurrence_against_numpy_slogdet(dll, n):
    """The sign is numpy's; |logabsdet - numpy's| <= 1e-4 * max(1, |numpy's|) for the fp32 families (the reference
    arithmetic measured on the CPU: at most 2.9e-6, a 30-fold margin)."""
    for kind, a in zip(KINDS, family_members(n)):
        x, st, piv, swp = mirror(dll, a)
        m, e = frexp_det(a, piv, swp)
        assert st == 0 and 0.5 <= abs(m) < 1.0
        sign, logabs = np.linalg.slogdet(a.astype(np.float64))
        mine = math.log(abs(m)) + e * math.log(2.0)
        print(f"n {n} {kind}: logabsdet {mine:.9g}, numpy {logabs:.9g}, diff {abs(mine - logabs):.3g}")
        assert math.copysign(1.0, m) == sign, (n, kind)
        assert abs(mine - logabs) <= 1e-4 * max(1.0, abs(logabs)), (n, kind, mine, logabs)


def test_recurrence_exact_cases(dll):
    for n in (2, 7, 20, 64, 65, 128):
        for odd in (False, True):
            a = permutation_matrix(n, odd)
            x, st, piv, swp = mirror(dll, a)
            assert st == 0 and frexp_det(a, piv, swp) == (-0.5 if odd else 0.5, 1), (n, odd)
            assert round(np.linalg.det(a.astype(np.float64))) == (-1 if odd else 1)
    for n in (64, 128):
        for k, dtype in ((100, np.float32), (-120, np.float32), (1000, np.float64), (-1000, np.float64)):
            a = np.diag(np.full(n, 2.0 ** k)).astype(dtype)
            x, st, piv, swp = mirror(dll, a)
            assert st == 0 and frexp_det(a, piv, swp) == (0.5, k * n + 1), (n, k)


def test_helpers_on_cpu_tensors():
    torch = pytest.importorskip("torch")
    mant = torch.tensor([0.5, -0.75, 0.0, math.nan, 0.625], dtype=torch.float64)
    exp = torch.tensor([1, 3, 0, 0, 12801], dtype=torch.int32)
    sign, logabs = g.slogdet_from_frexp(mant, exp)
    assert sign.dtype == torch.float64 and logabs.dtype == torch.float64
    assert sign[:3].tolist() == [1.0, -1.0, 0.0] and math.isnan(sign[3].item()) and sign[4].item() == 1.0
    assert logabs[0].item() == 0.0                                              # log 0.5 + ln 2
    assert logabs[1].item() == pytest.approx(math.log(6.0), rel=1e-15)
    assert logabs[2].item() == -math.inf and math.isnan(logabs[3].item())
    assert logabs[4].item() == pytest.approx(math.log(0.625) + 12801 * math.log(2.0), rel=1e-15)
    det = g.det_from_frexp(mant, exp)
    assert det.dtype == torch.float64
    assert det[:3].tolist() == [1.0, -6.0, 0.0] and math.isnan(det[3].item()) and det[4].item() == math.inf   # overflows
    assert g.det_from_frexp(mant[:2], exp[:2], torch.float32).dtype == torch.float32
    # a pair whose value is a double although 2**exp alone is not
    big = g.det_from_frexp(torch.tensor([0.5], dtype=torch.float64), torch.tensor([1024], dtype=torch.int32))
    assert big.item() == 2.0 ** 1023
    tiny = g.det_from_frexp(torch.tensor([0.5], dtype=torch.float64), torch.tensor([-1073], dtype=torch.int32))
    assert tiny.item() == 2.0 ** -1074
    m, e = np.frexp(np.array([3.0, -1e-300, 7e250]))
    back = g.det_from_frexp(torch.from_numpy(m), torch.from_numpy(e.astype(np.int32)))
    assert same_doubles(back.numpy(), np.array([3.0, -1e-300, 7e250]))
