"""Inputs and checkers for the pivoted fp64 paths (tests/test_fp64_cases.py proves them on the CPU,
tests/test_gpu_fp64_pivoted.py runs them on the blocked fp64 path and on the fp64 sweep).  Pure numpy, host only.

Three things live here:

  * ``dist_matrix64``: the input distributions of test_gpu_parity.dist_matrix (gate / ref100 / rand / hollow),
    generated in fp32 as there and widened, so that every entry is the same number in both precisions;
  * ``tie_matrix64``: inversions whose pivot search meets EXACT ties at chosen rows and columns.  A gate-like base
    (U(-1,1) + sqrt(n) I with a quarter of the rows swapped in pairs: steps that swap and steps that do not) in which
    both rows of a pair (j, r1, r2) are zero before column j and hold +-4096 in column j.  A row whose entries in the
    earlier pivot columns are zero has zero multipliers in those steps (skipped) and zero factors in the delayed
    rank-bw updates (fma(0, x, old) = old), so at step j the two rows still hold exactly +-4096, far above every
    other candidate, and the search must break the tie by position: the lowest row wins.  Both rows lie below
    position j (or r1 sits on the diagonal, r1 == j: no swap may happen then), so no earlier step moves them;
  * ``reference_inverse`` / ``forward_bound``: a reference that shares nothing with the elimination under test
    (numpy.linalg.inv polished by two Newton steps in extended precision) and the fp64 forward-error bound.
"""
import functools

import numpy as np

from conftest import gate_matrix

TIE_VALUE = 4096.0
U64 = 2.0 ** -53  # unit roundoff of float64


def dist_matrix64(kind, n, seed):
    """test_gpu_parity.dist_matrix in float64: the same fp32-representable entries."""
    rng = np.random.default_rng(seed)
    if kind == "gate":
        return gate_matrix(n, seed).astype(np.float64)
    if kind not in ("ref100", "rand", "hollow"):
        raise ValueError(kind)
    a = rng.uniform(0, 1 if kind == "rand" else 100, (n, n))
    if kind == "hollow":
        np.fill_diagonal(a, 0.0)
    return a.astype(np.float32).astype(np.float64)


# ---- exact ties -----------------------------------------------------------------------------------------------------
def tie_matrix64(n, pairs, seed):
    """float64 matrix with one exact two-way tie per entry (j, r1, r2) of ``pairs``: rows r1 < r2 are zero before
    column j, row r1 holds +4096 in column j and row r2 +4096 (even position in the list) or -4096 (odd position)."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, (n, n)) + np.sqrt(n) * np.eye(n)
    idx = rng.permutation(n)[: (n // 4) & ~1].reshape(-1, 2)
    a[np.concatenate([idx[:, 0], idx[:, 1]])] = a[np.concatenate([idx[:, 1], idx[:, 0]])]
    used = set()
    for k, (j, r1, r2) in enumerate(pairs):
        assert 0 <= j <= r1 < r2 < n, (j, r1, r2)          # below position j, or r1 on the diagonal
        assert not {r1, r2} & used, (j, r1, r2)             # a row belongs to one pair
        used |= {r1, r2}
        for r, sign in ((r1, 1.0), (r2, -1.0 if k % 2 else 1.0)):
            a[r] = rng.uniform(-1.0, 1.0, n)
            a[r, :j] = 0.0
            a[r, j] = sign * TIE_VALUE
    return a


def column_at_step(a, j):
    """Column j over the rows >= j as it stands when step j searches it, by a plain float64 elimination with partial
    pivoting (first maximum) of the first j columns.  Only the rows below the pivot are eliminated: the candidates of
    a later column do not depend on what Gauss-Jordan does above the diagonal.  The second value is the row order:
    entry i is the input row that sits at position i by then."""
    m = np.array(a, dtype=np.float64)
    n = m.shape[0]
    pos = np.arange(n)
    for r in range(j):
        p = r + int(np.argmax(np.abs(m[r:, r])))
        if p != r:
            m[[r, p]] = m[[p, r]]
            pos[[r, p]] = pos[[p, r]]
        f = m[r + 1:, r] / m[r, r]
        m[r + 1:, r + 1:] -= f[:, None] * m[r, r + 1:][None, :]
        m[r + 1:, r] = 0.0
    return m[j:, j].copy(), pos


# Placements.  Blocked fp64 path at these orders: TR = 8 rows per workgroup of the step kernel, one arg-max record per
# row tile, bw = 64 or 128 (default).  Distances: +1 inside one row tile (folded through LDS), +8 adjacent tiles and
# +64 (folded by the record loop and the wave reduction of the next launch).  Columns: 0, bw - 1 (last step of a
# block: the records of column bw come from the prep kernel after the rank-bw update), bw, the middle of the second
# block, and one pair with r1 == j.  Signs alternate down the list: equal, opposite, equal, ...
TIES_300 = [(0, 8, 9), (63, 70, 78), (64, 100, 164), (96, 96, 97), (127, 200, 208), (128, 130, 194), (192, 210, 211)]
# N = 2100 pads to 2176 rows at bw = 128: 272 row tiles, so the record loop of the step kernel (256 threads) takes a
# second turn and rows 2048 apart meet in ONE thread, the higher row second.
TIES_2100 = [(0, 3, 2051), (5, 5, 2053), (127, 136, 137), (128, 1000, 1064), (200, 300, 2090)]
# fp64 sweep at N = 1100: TR = 4 (275 row tiles: rows 1024 apart meet in one thread of the record loop) and two
# column tiles of 1024 columns: the pivot columns from 1024 on, and their records, belong to the second.
TIES_SWEEP_1100 = [(0, 2, 1026), (1, 8, 9), (2, 20, 24), (3, 3, 1027), (1030, 1040, 1041), (1050, 1050, 1054)]

# (name, n, pairs, seed): every tie matrix the GPU tests use
TIE_CASES = [("t300", 300, TIES_300, 64_300), ("t2100", 2100, TIES_2100, 64_2100), ("s1100", 1100, TIES_SWEEP_1100, 64_1100)]


@functools.lru_cache(maxsize=None)
def tie_case(name):
    """(matrix, pairs) of a TIE_CASES entry; the matrix is shared and read-only."""
    _, n, pairs, seed = next(c for c in TIE_CASES if c[0] == name)
    a = tie_matrix64(n, pairs, seed)
    a.setflags(write=False)
    return a, pairs


# ---- the independent reference ---------------------------------------------------------------------------------------
def longdouble_eps():
    return float(np.finfo(np.longdouble).eps)


def longdouble_is_extended():
    """True where np.longdouble carries at least 64 significand bits (x87 extended or wider): eps below 2^-60."""
    return longdouble_eps() < 2.0 ** -60


def norm_inf(m):
    return np.abs(m).sum(axis=1).max()


def residual_inf_longdouble(a, x):
    """||A X - I||_inf with the product and the sums in np.longdouble."""
    n = a.shape[0]
    r = np.asarray(a, np.longdouble) @ np.asarray(x, np.longdouble).reshape(n, n)
    r[np.diag_indices(n)] -= 1
    return norm_inf(r)


def reference_inverse(a):
    """inv(A) in np.longdouble: numpy.linalg.inv in float64, then two Newton steps X <- X + X (I - A X) carried out
    in longdouble.  One step squares ||I - A X|| (about kappa 2^-53 to begin with), so two leave the rounding of the
    longdouble products: far below what a float64 result is compared at."""
    a = np.asarray(a, dtype=np.float64)
    n = a.shape[0]
    al = a.astype(np.longdouble)
    x = np.linalg.inv(a).astype(np.longdouble)
    eye = np.eye(n, dtype=np.longdouble)
    for _ in range(2):
        x = x + x @ (eye - al @ x)
    return x


def kappa_inf(a, xref):
    return float(norm_inf(np.asarray(a, np.longdouble)) * norm_inf(xref))


def forward_bound(a, xref, factor=1.0):
    """fp64 counterpart of conftest.forward_tolerance: max|X - Xref| / max|Xref| <= factor * kappa_inf(A) * 2^-53,
    kappa_inf = ||A||_inf ||Xref||_inf.

    F = 1 comes from the reference-order oracle (oracle.matrix_inv_64, one fma per element and step), not from the
    kernels under test: on every input of REFERENCE_CASES its error against reference_inverse is at most
    0.151 kappa_inf 2^-53 (worst: gate, N = 300; 0.128 and 0.116 on gate at 257 and 520, at most 0.026 on the three
    U(0, .) kinds; numpy.linalg.inv: at most 0.044), and tests/test_fp64_cases.py keeps it at or below F / 4 on each."""
    return factor * kappa_inf(a, xref) * U64


def forward_error(x, xref):
    n = xref.shape[0]
    d = np.asarray(x, np.longdouble).reshape(n, n) - xref
    return float(np.abs(d).max() / np.abs(xref).max())


# (kind, n) the GPU tests compare with the reference; one seed rule for both test modules
REFERENCE_KINDS = ("gate", "ref100", "rand", "hollow")
REFERENCE_ORDERS = (257, 300, 520)
REFERENCE_CASES = [(kind, n) for n in REFERENCE_ORDERS for kind in REFERENCE_KINDS]


@functools.lru_cache(maxsize=None)
def reference_case(kind, n):
    """(A, Xref) of a REFERENCE_CASES entry, computed once per process; both read-only."""
    a = dist_matrix64(kind, n, 64_000 + n)
    xref = reference_inverse(a)
    a.setflags(write=False)
    xref.setflags(write=False)
    return a, xref
