"""CPU checks of the solve tests' own expected values (no device).  tests/solve_mirror.c restates Gauss-Jordan on
[A | B]; with B = I the augmented columns are the explicit right half of [A | I], so X must be the oracle's inverse bit
for bit -- that pins the mirror's pivot rule, division, fused multiply-adds and zero-multiplier skip to the oracle's.
The columns of B never meet one another, so solving them together or one by one must not change a bit either."""
import numpy as np
import pytest

from det_cases import MIRROR_ORDERS, NOPIVOT_ORDERS, dominant_member, family_members
from resident_cases import TIE_ORDERS, tie_batch
from solve_cases import build_solve_mirror, mirror_solve, rhs


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return build_solve_mirror(tmp_path_factory.mktemp("solve_mirror"))


@pytest.mark.parametrize("n", MIRROR_ORDERS)
def test_identity_gives_the_oracles_inverse(oracle, dll, n):
    for a in family_members(n):
        want, info = oracle.matrix_inv_32(a, n, return_info=True)
        x, st = mirror_solve(dll, a, np.eye(n, dtype=np.float32))
        assert st == info["status"] == 0
        assert np.array_equal(x.reshape(-1), want), n
        a64 = a.astype(np.float64) * 1.000000001  # entries that are no float32 values
        want, info = oracle.matrix_inv_64(a64, n, return_info=True)
        x, st = mirror_solve(dll, a64, np.eye(n))
        assert st == info["status"] == 0
        assert np.array_equal(x.reshape(-1), want), n


@pytest.mark.parametrize("n", NOPIVOT_ORDERS)
def test_identity_gives_the_oracles_inverse_without_pivoting(oracle, dll, n):
    for dtype in (np.float32, np.float64):
        a = dominant_member(n, dtype)
        want, info = oracle.matrix_inversion_no_pivots(a, n, return_info=True)
        x, st = mirror_solve(dll, a, np.eye(n, dtype=dtype), pivoting=False)
        assert st == info["status"] == 0
        assert np.array_equal(x.reshape(-1), want), (n, dtype)


@pytest.mark.parametrize("n", MIRROR_ORDERS)
def test_columns_are_independent(dll, n):
    k = 11
    for dtype in (np.float32, np.float64):
        for a in family_members(n, dtype):
            b = rhs(n, k, 40 + n, dtype)
            x, st = mirror_solve(dll, a, b)
            assert st == 0
            for c in range(k):
                xc, stc = mirror_solve(dll, a, b[:, c:c + 1])
                assert stc == 0 and np.array_equal(xc[:, 0], x[:, c]), (n, dtype, c)


@pytest.mark.parametrize("n", TIE_ORDERS)
def test_ties(oracle, dll, n):
    for a in tie_batch(n):
        want, info = oracle.matrix_inv_32(a, n, return_info=True)
        x, st = mirror_solve(dll, a, np.eye(n, dtype=np.float32))
        assert st == info["status"]
        if st == 0:
            assert np.array_equal(x.reshape(-1), want)


def test_bad_input_is_flagged(dll):
    a = family_members(20)[0]
    b = rhs(20, 3, 5)
    assert mirror_solve(dll, a, b)[1] == 0
    nan_b = b.copy()
    nan_b[7, 1] = np.nan
    x, st = mirror_solve(dll, a, nan_b)
    assert st == 2
    # the elimination goes on regardless: the NaN stays in its own column
    good, _ = mirror_solve(dll, a, b)
    assert np.array_equal(x[:, [0, 2]], good[:, [0, 2]]) and np.isnan(x[:, 1]).any()
    inf_b = b.copy()
    inf_b[0, 0] = np.inf
    assert mirror_solve(dll, a, inf_b)[1] == 2
    assert mirror_solve(dll, np.ones((20, 20), np.float32), b)[1] == 2      # rank 1: an exactly zero pivot
    assert mirror_solve(dll, np.zeros((5, 5)), rhs(5, 2, 1, np.float64))[1] == 2
    nan_a = a.copy()
    nan_a[4, 7] = np.nan
    assert mirror_solve(dll, nan_a, b)[1] == 2
    hit = dominant_member(20, np.float32)
    hit[1, 1] = hit[1, 0] = 0.0                                             # stays exactly zero without pivoting
    assert mirror_solve(dll, hit, b, pivoting=False)[1] == 2
