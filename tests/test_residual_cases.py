"""CPU-only proof that the cases of tests/residual_cases.py are what they claim to be: the oracle's three metrics equal
the int64 answers and the closed forms, and the oracle alone stays inside ``float_tolerances`` of a float64 product.
A precondition of tests/test_gpu_residual.py."""
import numpy as np
import pytest

from residual_cases import (FLOAT_ORDERS, ORDERS, ORDERS_SCALAR, ORDERS_VECTOR, all_positions, edge_indices, edge_positions,
                            expected_exact, float_inputs, float_tolerances, frobenius_tolerance_exact, integer_batch,
                            integer_pair, planted, planted_batch, proof_positions, sum_squares_exact)


def oracle_three(oracle, a, x):
    n = a.shape[0]
    return oracle.residual_inf(a, x, n), oracle.residual_inf_left(a, x, n), oracle.frobenius_metric(a, x, n)


def test_order_lists():
    assert all(n & 3 for n in ORDERS_SCALAR) and not any(n & 3 for n in ORDERS_VECTOR)
    assert len(ORDERS) == len(set(ORDERS)) == len(ORDERS_SCALAR) + len(ORDERS_VECTOR)
    # both branches on each side of the 64-tile edge and of the 2 x 2 / 3 x 3 workgroup edge
    assert {63, 65, 127, 129} <= set(ORDERS_SCALAR) and {60, 64, 68, 128, 132} <= set(ORDERS_VECTOR)
    assert edge_indices(1) == [0] and edge_indices(16) == [0, 15] and edge_indices(17) == [0, 15, 16]
    assert edge_indices(130) == [0, 15, 16, 31, 32, 47, 48, 63, 64, 79, 80, 95, 96, 111, 112, 127, 128, 129]
    assert len(all_positions(65)) == 4225 and len(all_positions(68)) == 4624
    assert set(proof_positions(130)) <= set(edge_positions(130))


@pytest.mark.parametrize("n", ORDERS)
def test_integer_pair_is_exact_on_the_oracle(oracle, n):
    a, x = integer_pair(n, 7)
    assert a.dtype == x.dtype == np.float32 and np.abs(x).max() <= 8 and np.abs(a[:n - 1]).max(initial=0) <= 8
    if n >= 8:
        assert not np.array_equal(a, a.T) and not np.array_equal(a @ x, np.eye(n)) and not np.array_equal(a, x)
    want = expected_exact(a, x)
    got = oracle_three(oracle, a, x)
    assert got[0] == want[0] and got[1] == want[1], (n, got, want)
    assert abs(got[2] - want[2]) <= frobenius_tolerance_exact(a, x), (n, got[2], want[2])
    # swapped operands swap the two norms
    swapped = expected_exact(x, a)
    assert swapped[:2] == (want[1], want[0])
    if n >= 16:
        # the worst row of A X - I is the last one (the scaled row), in the last partial tile
        c = a.astype(np.int64) @ x.astype(np.int64) - np.eye(n, dtype=np.int64)
        assert int(np.abs(c).sum(axis=1).argmax()) == n - 1


def test_integer_batch_matches_the_single_form():
    a, x = integer_batch(5, 7, 3)
    want = expected_exact(a, x)
    assert want.shape == (7, 3) and len({tuple(w) for w in want}) == 7
    for b in range(7):
        assert tuple(want[b]) == expected_exact(a[b], x[b])
    assert np.array_equal(sum_squares_exact(a, x), [sum_squares_exact(a[b], x[b]) for b in range(7)])


@pytest.mark.parametrize("delta", [1.0, 2.0 ** -20], ids=["1", "2^-20"])
@pytest.mark.parametrize("n", ORDERS)
def test_planted_closed_forms_equal_the_oracle(oracle, n, delta):
    for i, j in proof_positions(n):
        a, x, (right, left) = planted(n, 11, i, j, delta)
        assert a.dtype == x.dtype == np.float32
        got = oracle_three(oracle, a, x)
        assert got[0] == right and got[1] == left, (n, i, j, got, right, left)
        # the closed forms for this A: one or two unit entries in a column, and in a row
        assert right == delta and left == (delta if j == 0 else 2 * delta)


def test_planted_batch_is_the_single_form():
    pos = edge_positions(33)
    a, x, want = planted_batch(33, 11, pos, 2.0 ** -20)
    assert a.shape == x.shape == (len(pos), 33, 33) and want.shape == (len(pos), 2)
    for b in (0, 7, len(pos) - 1):
        a1, x1, w1 = planted(33, 11, pos[b][0], pos[b][1], 2.0 ** -20)
        assert np.array_equal(a[b], a1) and np.array_equal(x[b], x1) and tuple(want[b]) == w1
    _, x0, _ = planted_batch(33, 11, pos, 0.0)
    assert (np.count_nonzero(x != x0, axis=(1, 2)) == 1).all()


@pytest.mark.parametrize("n", FLOAT_ORDERS)
def test_oracle_is_within_float_tolerances_of_a_float64_product(oracle, n):
    for name, a in float_inputs(n).items():
        x, info = oracle.matrix_inv_32_inplace(a, n, return_info=True)
        assert info["status"] == 0, (n, name)
        x = x.reshape(n, n)
        a64, x64 = a.astype(np.float64), x.astype(np.float64)
        got = oracle_three(oracle, a, x)
        eye = np.eye(n)
        c = a64 @ x64
        want = (np.abs(c - eye).sum(axis=1).max(), np.abs(x64 @ a64 - eye).sum(axis=1).max(),
                np.sqrt(float(n)) - np.sqrt((c * c).sum()))
        tol_r, tol_f = float_tolerances(a, x)
        tol_l, _ = float_tolerances(x, a)
        assert abs(got[0] - want[0]) <= tol_r, (n, name, got[0], want[0], tol_r)
        assert abs(got[1] - want[1]) <= tol_l, (n, name, got[1], want[1], tol_l)
        assert abs(got[2] - want[2]) <= tol_f, (n, name, got[2], want[2], tol_f)
        # the bounds are far below what they judge
        assert tol_r < 1e-2 * want[0] and tol_l < 1e-2 * want[1], (n, name, tol_r, want[0], tol_l, want[1])
