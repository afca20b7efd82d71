"""Degenerate and exactly invertible inputs (tests/test_degenerate_cases.py proves them on the CPU oracle,
tests/test_gpu_degenerate.py runs them on every GPU path).  Pure numpy, seeded; every generator takes the dtype.

Three kinds:
  * singular by construction (``zero_column``, ``zero_row``, ``ones_block``, the status-2 part of ``OVERFLOW_LIST``):
    the bad pivot is met late in the elimination, not at step 0 or 1;
  * exact and non-singular (``signed_pow2_permutation``, ``pow2_diagonal``, ``unit_bidiagonal``, ``block_diagonal``):
    every Gauss-Jordan intermediate is exact in fp32 and fp64, so there is one right answer whatever the blocking or
    update order, and the generator writes it down itself -- no solver computes it;
  * near-singular (``duplicate_rows``): status 0 with a huge, finite inverse in fp32.
"""
import numpy as np

from conftest import gate_matrix

STATUS_OK = 0
STATUS_SINGULAR = 2


def canon(x):
    """``conftest.canonical_bytes`` that keeps the dtype: the bytes of x with -0.0 stored as +0.0 (for a float32
    array the very same bytes as canonical_bytes)."""
    x = np.ascontiguousarray(x).reshape(-1)
    assert x.dtype in (np.float32, np.float64)
    return (x + x.dtype.type(0.0)).tobytes()


# ---- singular by construction ---------------------------------------------------------------------------------------
def zero_column(n, k, seed, dtype=np.float32, base=None):
    """gate_matrix with column k zero: the column stays exactly zero, so the bad pivot is met at step k.  (``base``:
    that very gate_matrix(n, seed), where a caller makes several inputs from one.)"""
    a = gate_matrix(n, seed).astype(dtype) if base is None else base.astype(dtype)
    a[:, k] = 0
    return a


def zero_row(n, r, seed, dtype=np.float32, base=None):
    """gate_matrix with row r zero: that row loses every search, so the failure comes at the last step."""
    a = gate_matrix(n, seed).astype(dtype) if base is None else base.astype(dtype)
    a[r, :] = 0
    return a


def ones_block(n, k, seed, dtype=np.float32):
    """diag(gate(k), [[1, 1], [1, 1]], gate(n - k - 2)): step k is a two-way tie that the lowest row wins, row k + 1
    then becomes exactly zero and step k + 1 finds an all-zero candidate column."""
    assert 0 <= k <= n - 2
    a = np.zeros((n, n), dtype)
    if k:
        a[:k, :k] = gate_matrix(k, seed)
    a[k:k + 2, k:k + 2] = 1
    if n - k - 2:
        a[k + 2:, k + 2:] = gate_matrix(n - k - 2, seed + 1)
    return a


OVERFLOW_MODES = ("rows", "cols", "both", "hollow")


def overflow(n, seed, mode, k):
    """fp32 only.  A gate_matrix ("rows", "cols", "both") or a hollow U(0, 100) matrix ("hollow") in which every
    row and / or column is scaled by 2^+k or 2^-k (a seeded coin per row / column), 60 <= k <= 127.  The entries
    stay finite (asserted); whether an intermediate overflows depends on the draw: OVERFLOW_LIST holds both outcomes."""
    assert mode in OVERFLOW_MODES and 60 <= k <= 127
    rng = np.random.default_rng([seed, n, k, OVERFLOW_MODES.index(mode)])
    if mode == "hollow":
        a = rng.uniform(0, 100, (n, n))
        np.fill_diagonal(a, 0.0)
    else:
        a = gate_matrix(n, seed).astype(np.float64)
    if mode in ("rows", "both", "hollow"):
        a = a * np.ldexp(1.0, k * rng.choice([-1, 1], n))[:, None]
    if mode in ("cols", "both", "hollow"):
        a = a * np.ldexp(1.0, k * rng.choice([-1, 1], n))[None, :]
    with np.errstate(over="ignore"):
        a = a.astype(np.float32)
    assert np.isfinite(a).all(), (n, seed, mode, k)
    return a


# (n, seed, mode, k, the oracle's status): chosen on the CPU oracle so that both outcomes occur at every order;
# tests/test_degenerate_cases.py asserts every status here against the oracle, both forms.
OVERFLOW_LIST = [
    (8, 0, "rows", 120, 0), (8, 0, "cols", 64, 0), (8, 1, "cols", 80, 2), (8, 2, "cols", 120, 2),
    (8, 0, "both", 60, 0), (8, 1, "hollow", 60, 0), (8, 2, "rows", 63, 0), (40, 0, "rows", 120, 0),
    (40, 1, "cols", 64, 0), (40, 2, "cols", 80, 2), (40, 0, "cols", 120, 2), (40, 1, "both", 60, 0),
    (40, 2, "hollow", 60, 0), (40, 2, "rows", 63, 0), (100, 0, "rows", 120, 0), (100, 2, "cols", 64, 0),
    (100, 0, "cols", 80, 2), (100, 1, "cols", 120, 2), (100, 2, "both", 60, 0), (100, 0, "hollow", 60, 2),
    (100, 2, "rows", 63, 0), (200, 0, "rows", 120, 0), (200, 0, "cols", 64, 0), (200, 1, "cols", 80, 2),
    (200, 2, "cols", 120, 2), (200, 0, "both", 60, 0), (200, 1, "hollow", 60, 2), (200, 2, "rows", 63, 0),
]


# ---- exact and non-singular: (matrix, expected inverse) --------------------------------------------------------------
def signed_pow2_permutation(n, seed, dtype=np.float32, negative_zeros=False):
    """a[i, p[i]] = +-2^e, e in [-40, 40]; the inverse is x[p[i], i] = 1 / a[i, p[i]].  With ``negative_zeros`` every
    zero of the input is -0.0: all candidates but one tie at a zero key, whatever its sign."""
    rng = np.random.default_rng([seed, n])
    p = rng.permutation(n)
    v = np.ldexp(rng.choice([-1.0, 1.0], n), rng.integers(-40, 41, n))
    a = np.full((n, n), -0.0 if negative_zeros else 0.0, dtype)
    x = np.zeros((n, n), dtype)
    a[np.arange(n), p] = v
    x[p, np.arange(n)] = 1.0 / v
    return a, x


def pow2_diagonal(n, dtype=np.float32):
    """diag(2^e) with the exponents spread over -100 ... 100 (fp32) or -900 ... 900 (fp64), in a fixed shuffled order."""
    top = 100 if np.dtype(dtype) == np.float32 else 900
    e = np.rint(np.linspace(-top, top, n)).astype(np.int64)
    e = e[np.random.default_rng(n).permutation(n)]
    return np.diag(np.ldexp(1.0, e)).astype(dtype), np.diag(np.ldexp(1.0, -e)).astype(dtype)


def unit_bidiagonal(n, seed, dtype=np.float32, upper=False):
    """I plus a +-1 sub-diagonal (``upper``: super-diagonal).  The inverse is the closed form
    x[i, j] = (-1)^(i-j) s[j] ... s[i-1] for i >= j, all entries in {-1, 0, 1}; a @ x == I holds in integers."""
    s = np.random.default_rng([seed, n]).choice([-1, 1], max(n - 1, 0)).astype(np.int32)
    a = np.eye(n, dtype=np.int32)
    x = np.eye(n, dtype=np.int32)
    for i in range(1, n):
        a[i, i - 1] = s[i - 1]
        x[i, :i] = -s[i - 1] * x[i - 1, :i]
    # a @ x == I in integers, row by row: (a @ x)[i] = x[i] + s[i-1] x[i-1]
    ax = x.copy()
    ax[1:] += s[:, None] * x[:-1]
    assert np.array_equal(ax, np.eye(n, dtype=np.int32)) and np.abs(x).max() <= 1
    if upper:
        a, x = a.T, x.T
    return np.ascontiguousarray(a.astype(dtype)), np.ascontiguousarray(x.astype(dtype))


def block_diagonal(orders, seed, dtype=np.float32):
    """(matrix, blocks): gate_matrix blocks of the given orders on the diagonal, exact zeros elsewhere.  A pivot search
    never leaves its block (all other candidates are zero), so the inverse is the blocks' inverses on the diagonal."""
    blocks = [gate_matrix(n, seed + b).astype(dtype) for b, n in enumerate(orders)]
    return place_blocks(blocks), blocks


def place_blocks(blocks):
    n = sum(b.shape[0] for b in blocks)
    m = np.zeros((n, n), blocks[0].dtype)
    off = 0
    for b in blocks:
        k = b.shape[0]
        m[off:off + k, off:off + k] = b
        off += k
    return m


# ---- near-singular ---------------------------------------------------------------------------------------------------
def duplicate_rows(n, seed):
    """gate_matrix with the last row equal to the first (fp32): rounding leaves a tiny non-zero last pivot, so the
    oracle returns status 0 and a finite, huge inverse.  Nothing is asserted about the values but their bits."""
    a = gate_matrix(n, seed)
    a[n - 1] = a[0]
    return a


def exact_families(n, seed, dtype=np.float32, names=None):
    """{name: (matrix, expected inverse)} of the exact families that need no oracle, at order n (``names``: a subset)."""
    make = {
        "perm": lambda: signed_pow2_permutation(n, seed, dtype),
        "perm-0": lambda: signed_pow2_permutation(n, seed + 1, dtype, negative_zeros=True),
        "diag": lambda: pow2_diagonal(n, dtype),
        "lower": lambda: unit_bidiagonal(n, seed, dtype),
        "upper": lambda: unit_bidiagonal(n, seed + 1, dtype, upper=True),
    }
    return {name: make[name]() for name in (names or make)}
