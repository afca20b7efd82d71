"""CPU proof of tests/fp64_cases.py, before the GPU sees any of it: the Newton reference has converged, the forward
bound leaves the reference-order oracle a factor of four, every tie is still an exact tie when its step searches
the column, and on every tie matrix the blocked mirror takes the pivots of the reference-order oracle -- which is
what makes the mirror a valid judge of the tie-break rule (lowest row among equal maxima)."""
import numpy as np
import pytest

import fp64_cases as C

needs_extended = pytest.mark.skipif(not C.longdouble_is_extended(), reason="np.longdouble is not an extended format")


def test_the_input_distributions_are_those_of_the_fp32_parity_tests():
    for kind in C.REFERENCE_KINDS:
        a = C.dist_matrix64(kind, 40, 5)
        assert a.dtype == np.float64 and np.array_equal(a, a.astype(np.float32))
    assert (np.diag(C.dist_matrix64("hollow", 40, 5)) == 0).all()
    assert 0 <= C.dist_matrix64("rand", 40, 5).min() and C.dist_matrix64("rand", 40, 5).max() <= 1
    assert C.dist_matrix64("ref100", 40, 5).max() > 50
    with pytest.raises(ValueError):
        C.dist_matrix64("other", 4, 0)


@needs_extended
@pytest.mark.parametrize("kind,n", C.REFERENCE_CASES)
def test_reference_has_converged_and_the_oracle_keeps_a_quarter_of_the_bound(oracle, kind, n):
    a, xref = C.reference_case(kind, n)
    assert xref.dtype == np.longdouble and xref.shape == (n, n)
    kappa = C.kappa_inf(a, xref)
    res = C.residual_inf_longdouble(a, xref)
    assert res < 1e3 * n * C.longdouble_eps() * kappa, (float(res), kappa)
    bound = C.forward_bound(a, xref)
    got, info = oracle.matrix_inv_64(a, n, return_info=True)
    assert info["status"] == 0
    err = C.forward_error(got, xref)
    err_np = C.forward_error(np.linalg.inv(a), xref)
    print(f"{kind} N={n}: kappa_inf {kappa:.3e}, oracle {err / bound:.3f}, numpy {err_np / bound:.3f} of kappa 2^-53")
    assert err <= bound / 4, err / bound
    assert err_np <= bound / 4, err_np / bound


def test_checkers_notice_a_wrong_inverse():
    """forward_error and residual_inf_longdouble on a result that is off in one entry by 2^-30 relative."""
    a = C.dist_matrix64("gate", 60, 1)
    x = np.linalg.inv(a)
    xref = x.astype(np.longdouble)
    assert C.forward_error(x, xref) == 0
    i, j = np.unravel_index(np.abs(x).argmax(), x.shape)
    bad = x.copy()
    bad[i, j] *= 1 + 2.0 ** -30
    assert C.forward_error(bad, xref) == pytest.approx(2.0 ** -30, rel=1e-6)
    assert C.forward_error(bad, xref) > C.forward_bound(a, xref)
    assert C.residual_inf_longdouble(a, bad) > 100 * C.residual_inf_longdouble(a, x)


def test_tie_generator_rejects_rows_that_would_move_or_are_shared():
    with pytest.raises(AssertionError):
        C.tie_matrix64(50, [(10, 5, 20)], 0)    # a row above position j is swapped away before step j
    with pytest.raises(AssertionError):
        C.tie_matrix64(50, [(0, 5, 6), (1, 6, 7)], 0)
    a = C.tie_matrix64(50, [(4, 4, 9), (10, 20, 21)], 0)
    assert a.dtype == np.float64
    assert (a[[4, 9], :4] == 0).all() and a[4, 4] == C.TIE_VALUE and a[9, 4] == C.TIE_VALUE
    assert (a[[20, 21], :10] == 0).all() and a[20, 10] == C.TIE_VALUE and a[21, 10] == -C.TIE_VALUE


def test_placements_cover_what_the_gpu_tests_need():
    by = {name: (n, pairs) for name, n, pairs, _ in C.TIE_CASES}
    n, pairs = by["t300"]
    assert {r2 - r1 for _, r1, r2 in pairs} == {1, 8, 64}
    assert all(r1 // 8 == r2 // 8 for _, r1, r2 in pairs if r2 - r1 == 1)       # one row tile of 8
    for bw in (64, 128):                                                       # first / last step, prep seam, mid-block
        assert {0, bw - 1, bw, bw + bw // 2} <= {j for j, _, _ in pairs}
    assert any(r1 == j for j, r1, _ in pairs)
    n, pairs = by["t2100"]
    assert -(-n // 128) * 128 // 8 > 256                                       # 272 records: a second loop turn
    assert sum(r2 - r1 == 2048 for _, r1, r2 in pairs) == 2 and any(r1 == j for j, r1, _ in pairs)
    assert {0, 127, 128} <= {j for j, _, _ in pairs}
    n, pairs = by["s1100"]
    assert -(-n // 4) > 256 and n > 1024
    assert {1, 4, 1024} <= {r2 - r1 for _, r1, r2 in pairs}
    assert all(r1 // 4 == r2 // 4 for _, r1, r2 in pairs if r2 - r1 == 1)       # one row tile of 4
    assert any(j >= 1024 for j, _, _ in pairs) and any(r1 == j for j, r1, _ in pairs)
    assert all(len(pairs) >= 2 for _, pairs in by.values())                    # equal and opposite signs in every case


@pytest.mark.parametrize("name", [c[0] for c in C.TIE_CASES])
def test_every_tie_is_an_exact_tie_when_its_step_searches_the_column(name):
    a, pairs = C.tie_case(name)
    for k, (j, r1, r2) in enumerate(pairs):
        col, pos = C.column_at_step(a, j)
        assert pos[r1] == r1 and pos[r2] == r2, (j, r1, r2)                    # neither row has moved
        assert col[r1 - j] == C.TIE_VALUE and col[r2 - j] == (-C.TIE_VALUE if k % 2 else C.TIE_VALUE), (j, r1, r2)
        others = np.delete(np.abs(col), [r1 - j, r2 - j])
        assert others.max() < C.TIE_VALUE / 8, (j, float(others.max()))         # the two rows are THE maximum


@pytest.mark.parametrize("name", [c[0] for c in C.TIE_CASES])
def test_tie_matrices_invert_and_the_mirror_takes_the_reference_order_pivots(oracle, name):
    """Status 0 and equal pivot sequences on the reference-order oracle and on the blocked mirror at both block
    widths; each tie goes to the lower row (a swap with r1, none where r1 is the diagonal row); and the results
    agree to rounding: two fp64 eliminations with the same pivots, each within kappa_inf 2^-53 of the inverse by
    fp64_cases.forward_bound.  (The only place where the N = 2100 matrix meets the reference-order oracle: ~10 s.)"""
    a, pairs = C.tie_case(name)
    n = a.shape[0]
    tol = 2 * np.linalg.cond(a, np.inf) * C.U64
    want, info = oracle.matrix_inv_64(a, n, return_info=True)
    assert info["status"] == 0
    for j, r1, _ in pairs:
        assert info["pivots"][j] == r1, (j, r1, int(info["pivots"][j]))
    for bw in (64, 128):
        got, binfo = oracle.matrix_inv_64_blocked(a, n, bw, return_info=True)
        assert binfo["status"] == 0
        assert np.array_equal(binfo["pivots"], info["pivots"]), (bw, np.argwhere(binfo["pivots"] != info["pivots"])[:8].tolist())
        assert np.abs(got - want).max() <= tol * np.abs(want).max()
