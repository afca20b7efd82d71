"""Inputs for the residual verifier (``residual_tile_kernel`` / ``residual_finalize_kernel``, reached through
``Inverter.residual`` and ``matrix_multiply``) with answers that no product routine computes.
tests/test_residual_cases.py proves them on the CPU oracle, tests/test_gpu_residual.py runs them on the kernel.
Pure numpy, seeded.

Three kinds:
  * ``integer_pair``: two unrelated integer matrices.  Every product and every partial sum of the three outputs is an
    integer far below 2^53, so there is one right answer whatever the summation order, the tiling or the order of the
    kernel's atomics, and ``expected_exact`` gets it from int64 arithmetic;
  * ``planted``: an exact integer inverse with one wrong entry.  The two norms are closed forms in a column and a row
    of the matrix -- what the users of the verifier depend on: a wrong entry raises the residual by the right amount;
  * float operands, judged by ``float_tolerances``: a-priori bounds from the operands alone.
"""
import numpy as np

from conftest import gate_matrix
from degenerate_cases import unit_bidiagonal

# (n & 3) != 0: the scalar-load branch of the tile kernel
ORDERS_SCALAR = [1, 2, 3, 5, 15, 17, 31, 33, 47, 49, 63, 65, 127, 129, 130]
# (n & 3) == 0: the 16-byte-load branch; 12, 20, 60, 68, 100 and 132 end in a partial k-chunk
ORDERS_VECTOR = [4, 8, 12, 16, 20, 32, 48, 60, 64, 68, 100, 128, 132]
# The edges are the kernel's own: 16 (one MFMA tile and one k-chunk), 32 (one wave), 64 (one workgroup tile), 128 / 129
# (2 x 2 against 3 x 3 workgroups).
ORDERS = sorted(ORDERS_SCALAR + ORDERS_VECTOR)

U53 = 2.0 ** -53  # unit roundoff of double


# ---- exact integers ---------------------------------------------------------------------------------------------------
def integer_pair(n, seed):
    """(A, X) float32: independent integer entries in [-8, 8]; not inverses of each other, not symmetric.  The last row
    of A is multiplied by 16, so the worst row of A X - I is the last row of the last (partial) tile."""
    rng = np.random.default_rng([seed, n])
    a = rng.integers(-8, 9, (n, n))
    x = rng.integers(-8, 9, (n, n))
    a[n - 1] *= 16
    return a.astype(np.float32), x.astype(np.float32)


def integer_batch(n, batch, seed):
    """(A, X) of shape (batch, n, n): the same distribution as integer_pair, every member its own draw."""
    rng = np.random.default_rng([seed, n, batch])
    a = rng.integers(-8, 9, (batch, n, n))
    x = rng.integers(-8, 9, (batch, n, n))
    a[:, n - 1] *= 16
    return a.astype(np.float32), x.astype(np.float32)


def _as_int64(m):
    i = np.asarray(m).astype(np.int64)
    assert np.array_equal(i, np.asarray(m)), "integer operands only"
    return i


def sum_squares_exact(a, x):
    """S = sum_ij (A X)_ij^2 as a Python int (per member for (B, n, n) operands: an int64 array)."""
    c = np.einsum("...ij,...jk->...ik", _as_int64(a), _as_int64(x))
    s = (c * c).sum(axis=(-2, -1))
    assert np.all(s < 2 ** 53)
    return int(s) if s.ndim == 0 else s


def expected_exact(a, x):
    """The verifier's three outputs from int64 arithmetic: max_i sum_j |(A X - I)_ij|, the same for X A, and
    sqrt(n) - sqrt(sum (A X)_ij^2).  (n, n) operands give three floats, (B, n, n) operands a (B, 3) float64 array."""
    ai, xi = _as_int64(a), _as_int64(x)
    n = ai.shape[-1]
    eye = np.eye(n, dtype=np.int64)
    right = np.abs(np.einsum("...ij,...jk->...ik", ai, xi) - eye).sum(axis=-1).max(axis=-1)
    left = np.abs(np.einsum("...ij,...jk->...ik", xi, ai) - eye).sum(axis=-1).max(axis=-1)
    s = np.asarray(sum_squares_exact(a, x), dtype=np.float64)   # exact: S < 2^53
    out = np.stack([right.astype(np.float64), left.astype(np.float64), np.sqrt(float(n)) - np.sqrt(s)], axis=-1)
    return tuple(float(v) for v in out) if out.ndim == 1 else out


def frobenius_tolerance_exact(a, x):
    """2^-50 (sqrt(n) + sqrt(S)) for integer operands: with S exact on both sides, only two correctly rounded square
    roots (relative error 2^-53 each) and one subtraction (2^-53 of a result no larger than the sum of the two roots)
    separate two evaluations of sqrt(n) - sqrt(S): at most 2^-51 (sqrt(n) + sqrt(S)) between them."""
    n = np.asarray(a).shape[-1]
    return 2.0 ** -50 * (np.sqrt(float(n)) + np.sqrt(np.asarray(sum_squares_exact(a, x), dtype=np.float64)))


# ---- one wrong entry in an exact inverse ------------------------------------------------------------------------------
def planted(n, seed, i, j, delta):
    """(A, X', (right, left)): A = unit_bidiagonal(n, seed), X' its exact integer inverse with ``delta`` added to
    X[i, j].  The expected norms are closed forms, not products:
        A X' - I = delta A[:, i] e_j^T   ->  ||.||_inf = |delta| max_r |A[r, i]|
        X' A - I = delta e_i A[j, :]     ->  ||.||_inf = |delta| sum_c |A[j, c]|
    ``delta`` is a power of two times a small integer (1, 2^-20, ...), so X' is exact in float32 and both forms are
    exact in double."""
    a, x, want = planted_batch(n, seed, [(i, j)], delta)
    return a[0], x[0], (float(want[0, 0]), float(want[0, 1]))


def planted_batch(n, seed, positions, delta):
    """The batched form: member b has ``delta`` (a scalar, or one value per member) added at ``positions[b]``.
    Returns (A (B, n, n), X' (B, n, n), expected (B, 2) float64)."""
    a, x = unit_bidiagonal(n, seed)
    pos = np.asarray(positions, dtype=np.int64).reshape(-1, 2)
    b = pos.shape[0]
    d = np.broadcast_to(np.asarray(delta, dtype=np.float64), (b,))
    xs = np.broadcast_to(x, (b, n, n)).copy()
    changed = xs[np.arange(b), pos[:, 0], pos[:, 1]].astype(np.float64) + d
    xs[np.arange(b), pos[:, 0], pos[:, 1]] = changed.astype(np.float32)
    assert np.array_equal(xs[np.arange(b), pos[:, 0], pos[:, 1]].astype(np.float64), changed), "delta is lost in float32"
    a64 = np.abs(a.astype(np.float64))
    want = np.stack([np.abs(d) * a64.max(axis=0)[pos[:, 0]], np.abs(d) * a64.sum(axis=1)[pos[:, 1]]], axis=1)
    return np.broadcast_to(a, (b, n, n)).copy(), xs, want


def all_positions(n):
    return [(i, j) for i in range(n) for j in range(n)]


def edge_indices(n):
    """0, n - 1 and the index on each side of every multiple of 16 below n (the 16 / 32 / 64 boundaries of the MFMA
    tile, the wave tile and the workgroup tile that exist at this order)."""
    s = {0, n - 1}
    for b in range(16, n, 16):
        s.update((b - 1, b))
    return sorted(s)


def edge_positions(n):
    """The four corners and every pair of edge indices."""
    e = edge_indices(n)
    return [(i, j) for i in e for j in e]


def proof_positions(n):
    """The positions tests/test_residual_cases.py proves the closed forms at: the corners and one off-tile entry."""
    return sorted({(0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1), (min(63, n - 1), min(64, n - 1))})


# ---- float operands ---------------------------------------------------------------------------------------------------
def ref100_matrix(n, seed):
    """U(0, 100) float32: the reference scripts' own input distribution."""
    return np.random.default_rng(seed).uniform(0, 100, (n, n)).astype(np.float32)


FLOAT_ORDERS = [3, 5, 63, 65, 100, 130, 257, 300]


def float_inputs(n):
    """{name: matrix} of the float cases at order n; their inverses come from the elimination under test."""
    return {"gate": gate_matrix(n, 4000 + n), "ref100": ref100_matrix(n, 4100 + n)}


def float_tolerances(l, r):
    """(bound for ||L R - I||_inf, bound for sqrt(n) - ||L R||_F): how far two evaluations in double of these outputs
    may lie apart, from the operands alone (float64 on the CPU, never from the code under test).

    Every element of L R is an n-term inner product of exactly representable products: evaluated in double in any order
    its error is at most gamma_n |L||R|_ij, gamma_n = n u / (1 - n u), u = 2^-53 (Higham, Accuracy and Stability of
    Numerical Algorithms, 2nd ed., (3.5)).  Subtracting the identity adds u, and the n-term row sum in any order another
    gamma_n of the row sum, itself at most (|L||R|)_i plus 1.  Together below 2 n u ||  |L||R|  ||_inf to first order for
    one evaluation, 4 n u for the distance between two:
        inf-norm outputs:  4 n 2^-53 || |L| |R| ||_inf
    The Frobenius norm of the element errors is at most gamma_n || |L||R| ||_F, the n^2-term sum of squares is evaluated
    pairwise or in short chains, and the two square roots and the subtraction add at most 2 u (sqrt(n) + ||L R||_F):
        Frobenius metric:  4 n 2^-53 || |L| |R| ||_F + 4 2^-53 sqrt(n)
    """
    la = np.abs(np.asarray(l, dtype=np.float64))
    ra = np.abs(np.asarray(r, dtype=np.float64))
    n = la.shape[-1]
    p = la @ ra
    return (4.0 * n * U53 * float(p.sum(axis=1).max()),
            4.0 * n * U53 * float(np.sqrt((p * p).sum())) + 4.0 * U53 * float(np.sqrt(n)))
