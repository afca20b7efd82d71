"""CPU proof of tests/overflow_cases.py: every entry of the route table, on its reference alone, is an input that a
test cannot pass on by accident -- status 0 from a finite input, a mostly finite result, infinities and NaN in it --
and the two rules for a zero multiplier part exactly where the table says they do.  Run with ``-m "not gpu"``."""
import numpy as np
import pytest

import overflow_cases as C
import subnormal_cases as S
from degenerate_cases import canon

F32, F64 = np.float32, np.float64


def differing(x, y):
    """Entries that differ, NaN equal to NaN and -0.0 to +0.0."""
    with np.errstate(invalid="ignore"):
        return int((~((x == y) | (np.isnan(x) & np.isnan(y)))).sum())


@pytest.mark.parametrize("route", list(C.ROUTES))
def test_every_table_entry_meets_the_conditions_on_its_reference(oracle, route):
    ref, cases = C.ROUTES[route]
    assert cases
    for c in cases:
        a, n = C.matrix(c), C.order(c)
        assert a.shape == (n, n) and a.dtype == c.dtype and np.isfinite(a).all(), c
        for bw in C.widths_of(route, c):
            x, st = C.reference(oracle, c, ref, bw)
            share, infs, nans = C.counts(x)
            assert st == C.OK, (c, bw)
            assert share >= C.MIN_FINITE_SHARE, (c, bw, share)
            assert infs >= max(4, n / 8), (c, bw, infs)
            assert nans >= 1 or ref == "mirror64", (c, bw)     # waived on the fp64 blocked route only
        (skip, st_skip), (thru, st_thru) = C.reference(oracle, c, "skip"), C.reference(oracle, c, "through")
        assert st_skip == st_thru == C.OK, c
        if ref == "mirror64":           # the composite order is the reference there: neither step rule gives its result
            if c.kind == "block_diag":
                for bw in C.widths_of(route, c):
                    assert differing(C.reference(oracle, c, ref, bw)[0], skip) >= n, (c, bw)
            continue
        if c.kind == "block_diag":      # the rules part: a test against the wrong one fails
            assert differing(skip, thru) >= n, (c, differing(skip, thru))
            assert not C.same_with_nonfinite(skip, thru)
        else:                           # dense: no exact-zero multiplier, the non-finite pattern included
            assert differing(skip, thru) == 0 and C.same_with_nonfinite(skip, thru), c


def test_block_diag_layout():
    for c in C.ROUTES["blocked32_block_diag"][1] + C.ROUTES["nopivot64_blocked"][1]:
        if c.kind != "block_diag":
            continue
        a = C.matrix(c)
        k = c.n[0] if c.first else c.n[1]
        assert not a[:k, k:].any() and not a[k:, :k].any()
        small = a[:k, :k] if c.first else a[k:, k:]
        assert np.array_equal(small, C.rows_down(c.n[0], c.dtype, c.pivoting, c.s))
        tiny = np.abs(small).max(axis=1) < np.finfo(c.dtype).tiny
        assert np.array_equal(np.nonzero(tiny)[0], np.arange(1, c.n[0], 3))


def test_the_fp64_blocked_mirror_has_an_overflow_boundary_of_its_own(oracle):
    """n = 300, s = 1028: the composite order of the rank-bw update flags the input (status 2) at both widths while the
    step oracle inverts it with 97 % of the entries finite -- the GPU route has to follow the mirror there."""
    c = C.BLOCKED64_STATUS2
    x, st = C.reference(oracle, c, "skip")
    assert st == C.OK and C.counts(x)[0] >= 0.95
    for bw in C.F64_BLOCKED_WIDTHS:
        _, st = C.reference(oracle, c, "mirror64", bw)
        assert st == C.SINGULAR, bw


def test_modes_agree_on_the_finite_inputs_of_the_suite(oracle):
    """Where every intermediate is finite the two rules differ in the sign of a zero only: equal after ``canon``."""
    from conftest import gate_matrix
    from nopivot_cases import sparse_spd, spd, tridiagonal

    for dtype, fn in ((F32, oracle.matrix_inv_32_inplace), (F64, oracle.matrix_inv_64)):
        for a in [gate_matrix(n, 5 * n).astype(dtype) for n in (5, 64, 130)] + \
                 [S.matrix(f, n, dtype) for f in S.PIVOTED for n in (16, 100)] + \
                 [np.kron(np.eye(3), gate_matrix(7, 3)).astype(dtype)]:
            n = a.shape[0]
            (x, i), (y, j) = (fn(a, n, return_info=True, zeros=z) for z in ("skip", "through"))
            assert i["status"] == j["status"] == 0 and np.isfinite(x).all()
            assert x.dtype == dtype and canon(x) == canon(y) and np.array_equal(i["pivots"], j["pivots"]), (dtype, n)
        for a in [spd(100, 1, dtype), sparse_spd(200, 2, dtype), tridiagonal(33, dtype)] + \
                 [S.matrix(f, 100, dtype) for f in S.NOPIVOT]:
            n = a.shape[0]
            (x, i), (y, j) = (oracle.matrix_inversion_no_pivots(a, n, return_info=True, zeros=z) for z in ("skip", "through"))
            assert i["status"] == j["status"] == 0 and np.isfinite(x).all()
            assert x.dtype == dtype and canon(x) == canon(y), (dtype, n)


def test_default_mode_is_skip(oracle):
    c = C.case("block_diag", F32, (8, 8))
    a = C.matrix(c)
    x = oracle.matrix_inv_32_inplace(a, 16)
    assert C.same_with_nonfinite(x, C.reference(oracle, c, "skip")[0])
    with pytest.raises(KeyError):
        oracle.matrix_inv_32_inplace(a, 16, zeros="sometimes")


@pytest.mark.parametrize("dtype", [F32, F64], ids=["fp32", "fp64"])
def test_same_with_nonfinite_in_the_members_dtype(dtype):
    want = np.array([1.0, -0.0, np.inf, -np.inf, np.nan, 2.5], dtype)
    ok = want.copy()
    ok[1] = 0.0                                         # -0.0 is +0.0
    ok[4] = np.frombuffer(np.array([-np.nan], dtype).tobytes(), dtype)[0]   # every NaN is one value
    assert C.same_with_nonfinite(ok, want) and C.same_with_nonfinite(want.reshape(2, 3), want)
    for i, v in ((2, -np.inf), (3, np.inf), (4, np.inf), (2, np.nan), (0, np.nan), (5, np.nextafter(dtype(2.5), dtype(3))),
                 (0, np.inf)):
        bad = want.copy()
        bad[i] = v
        assert not C.same_with_nonfinite(bad, want), (i, v)
    assert not C.same_with_nonfinite(want[:5], want)
    assert not C.same_with_nonfinite(want.astype(F64 if dtype == F32 else F32), want)   # the dtype is part of it
    if dtype == F32:    # and on float32 it is the rule of subnormal_cases
        assert S.same_with_nonfinite(ok, want)
