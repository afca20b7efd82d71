"""The reference and the case builders of the block finder (``Inverter.csr_block_starts`` / ``csr_find_blocks``,
``mi32_csr_find_blocks_device``).  No pytest in here: the test files import what they need.

The reference is the definition of include/mat_inv_32_csr_find.h restated in NumPy with plain loops, step by step:

    nat[0] = 1;  nat[i] = 0 iff rows i - 1 and i hold the same column indices in stored order
    sv[i]  = nat[i] or (i - run(i)) % max_order == 0,       run(i) = the largest j <= i with nat[j]
    start  = sv, or with agglomeration the orbit of row 0 under
             next(i) = the largest p in (i, i + max_order] with (p == N or sv[p])

Integers only: every comparison against it is array equality.  A case is a namespace of ``n``, ``crow``, ``col``
(int64) and whatever the builder adds; every builder asserts on the host that its case has the property it is named
for.
"""
import functools
from types import SimpleNamespace

import numpy as np

from csr_cases import block_jacobi_case, csr_from_pairs, typed  # noqa: F401  (re-exported for the tests)

MAX_ORDERS = (1, 2, 8, 32, 127, 128)


# ---- the mirror --------------------------------------------------------------------------------------------------------
def mirror_nat(crow, col):
    n = crow.size - 1
    nat = np.zeros(n, np.uint8)
    nat[0] = 1
    for i in range(1, n):
        a, b = col[crow[i - 1]:crow[i]], col[crow[i]:crow[i + 1]]
        nat[i] = 0 if a.size == b.size and np.array_equal(a, b) else 1
    return nat


def mirror_sv(nat, max_order):
    sv = np.zeros(nat.size, np.uint8)
    run = 0
    for i in range(nat.size):
        if nat[i]:
            run = i
        sv[i] = 1 if nat[i] or (i - run) % max_order == 0 else 0
    return sv


def mirror_orbit(sv, max_order):
    n = sv.size
    start = np.zeros(n, np.uint8)
    i = 0
    while i < n:
        start[i] = 1
        p = min(i + max_order, n)
        while not (p == n or sv[p]):
            p -= 1
        i = p
    return start


def mirror_starts(crow, col, max_order, agglomerate, nat=None):
    """start[N] (uint8) of the definition; ``nat``: step 1 where the caller has it already."""
    assert 1 <= max_order <= 128 and crow.size >= 2
    nat = mirror_nat(crow, col) if nat is None else nat
    sv = mirror_sv(nat, max_order)
    return mirror_orbit(sv, max_order) if agglomerate else sv


def orders_of(start):
    """The block orders: the gaps between the ones, and from the last one to N."""
    return np.diff(np.flatnonzero(start), append=start.size).astype(np.int32)


def check_invariants(case, max_order):
    """What holds for every pattern; returns (starts without agglomeration, starts with it)."""
    loose = mirror_starts(case.crow, case.col, max_order, False, case.nat)
    merged = mirror_starts(case.crow, case.col, max_order, True, case.nat)
    for start in (loose, merged):
        orders = orders_of(start)
        assert start[0] == 1 and set(np.unique(start)) <= {0, 1}
        assert int(orders.sum()) == case.n and orders.min() >= 1 and orders.max() <= max_order
    assert (loose[merged == 1] == 1).all()          # merging only removes starts
    return loose, merged


# ---- building patterns ---------------------------------------------------------------------------------------------------
def _case(crow, col, **more):
    crow, col = np.asarray(crow, np.int64), np.asarray(col, np.int64)
    assert crow[0] == 0 and crow[-1] == col.size and (np.diff(crow) >= 0).all()
    return SimpleNamespace(n=crow.size - 1, crow=crow, col=col, nat=mirror_nat(crow, col), **more)


def from_rows(rows, **more):
    """The case whose row i stores the column indices rows[i], in that order."""
    crow = np.concatenate(([0], np.cumsum([len(r) for r in rows])))
    col = np.concatenate([np.asarray(r, np.int64) for r in rows]) if crow[-1] else np.zeros(0, np.int64)
    return _case(crow, col, **more)


def typed_pattern(case, idtype):
    return case.crow.astype(idtype), case.col.astype(idtype)


def common_pattern_case(n):
    """Every row stores the same three columns: one natural run of n rows."""
    case = from_rows([[0, n // 2, n - 1] if n > 2 else [0]] * n)
    assert case.nat.sum() == 1
    return case


def tridiagonal_case(n):
    """Every row differs from the one before: every supervariable is one row.  (n = 2 is two full rows: the diagonal
    alone there.)"""
    case = from_rows([[c for c in (i - 1, i, i + 1) if 0 <= c < n] if n > 2 else [i] for i in range(n)])
    assert case.nat.all()
    return case


@functools.lru_cache(maxsize=None)
def one_entry_case():
    """Pairs of rows that differ in one place only.  ``want_nat``: {row: nat} for the rows the case is about."""
    n = 1024
    base = [3, 40, 41, 100, 333, 500, 640, 900, 1001]
    long_row = list(range(10, 710))                                  # 700 entries: several rounds per group
    first, middle, last = list(base), list(base), list(base)
    first[0], middle[4], last[-1] = 2, 334, 1002
    long_last = list(long_row)
    long_last[-1] = 800
    rows = [base, base, first, base, middle, base, last, base, base + [1003], base,   # 0 ... 9
            [], base, [], [], base,                                                    # 10 ... 14
            long_row, long_row, long_last, long_row,                                   # 15 ... 18
            [3, 7], [7, 3], [3, 7], [3, 7]]                                            # 19 ... 22
    want = {1: 0, 2: 1, 3: 1, 4: 1, 5: 1, 6: 1, 7: 1, 8: 1, 9: 1,    # first / middle / last entry, one entry more
            10: 1, 11: 1, 12: 1, 13: 0, 14: 1,                        # empty rows, single and consecutive
            15: 1, 16: 0, 17: 1, 18: 1,                               # 700 entries, the last one differs
            19: 1, 20: 1, 21: 1, 22: 0}                               # the same set in another stored order
    rows += [[i] for i in range(len(rows), n)]                       # the rest: the diagonal, all different
    case = from_rows(rows, want_nat=want)
    assert case.n == n and int(case.col.max()) < n
    assert all(case.nat[i] == v for i, v in want.items())
    return case


def runs_case(run_lengths, seed, entries=5):
    """Natural runs of the given lengths: the rows of a run share ``entries`` sorted distinct columns, consecutive runs
    differ.  ``run_first``: the first row of every run."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(run_lengths, np.int64)
    n = int(lengths.sum())
    assert n > 4 * entries
    first = np.concatenate(([0], np.cumsum(lengths)[:-1]))
    offsets = np.cumsum(rng.integers(1, n // (2 * entries), (lengths.size, entries)), axis=1)     # distinct, below n
    patterns = np.sort((first[:, None] + offsets) % n, axis=1)
    col = patterns[np.repeat(np.arange(lengths.size), lengths)].reshape(-1)
    crow = np.arange(n + 1, dtype=np.int64) * entries
    case = _case(crow, col, run_first=first)
    assert np.array_equal(np.flatnonzero(case.nat), first)
    return case


def _lengths_with(n, fixed, rng, top):
    """Run lengths that sum to n: random ones of 1 ... top, but a run of fixed[f] rows starting at every row f."""
    lengths, at = [], 0
    for f in sorted(fixed) + [n]:
        while at < f:
            k = min(int(rng.integers(1, top + 1)), f - at)
            lengths.append(k)
            at += k
        if f < n:
            lengths.append(fixed[f])
            at += fixed[f]
    assert sum(lengths) == n
    return lengths


SEAM_KINDS = ("run", "block", "boundary")


@functools.lru_cache(maxsize=None)
def seams_case(chunk, max_order, kind):
    """N = three chunks and a prime remainder; over each of the first three seams s = chunk, 2 chunk, 3 chunk
    * ``run``:      a natural run longer than max_order, from s - max_order - 3 to s + max_order + 5
    * ``block``:    a block that starts max_order - 1 rows before s: a run of exactly max_order rows ends there, and
                    the rows from there on are all different
    * ``boundary``: a supervariable boundary exactly on s, between two runs
    and random runs elsewhere."""
    m = max_order
    assert chunk > 8 * m + 16 and kind in SEAM_KINDS
    n = 3 * chunk + 293
    rng = np.random.default_rng(7100 + m)
    fixed = {}
    for s in (chunk, 2 * chunk, 3 * chunk):
        if kind == "run":
            fixed[s - m - 3] = 2 * m + 8
        elif kind == "block":
            q = s - (m - 1)
            fixed[q - m] = m
            for i in range(q, q + m + 2):
                fixed[i] = 1
        else:
            fixed[s - 3] = 3
            fixed[s] = 2
    case = runs_case(_lengths_with(n, fixed, rng, max(1, min(m, 40))), 7200 + m)
    assert case.n == n
    sv = mirror_sv(case.nat, m)
    merged = mirror_orbit(sv, m)
    for s in (chunk, 2 * chunk, 3 * chunk):
        if kind == "run":
            assert case.nat[s - m - 3] and not case.nat[s - m - 2:s + m + 5].any() and case.nat[s + m + 5]
        elif kind == "block":
            q = s - (m - 1)
            assert merged[q] == 1 and merged[q + 1:q + m].sum() == 0 and merged[q + m] == 1 and q <= s < q + m
        else:
            assert case.nat[s] and sv[s]
    return case


def stencil27_case(grid, dof):
    """A 27-point stencil on the grid with ``dof`` unknowns per node: the rows of a node share the node's pattern (the
    unknowns of every neighbouring node, sorted), and neighbouring nodes differ."""
    nx, ny, nz = grid
    rows = []
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                nodes = sorted((x + dx) + nx * ((y + dy) + ny * (z + dz))
                               for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                               if 0 <= x + dx < nx and 0 <= y + dy < ny and 0 <= z + dz < nz)
                cols = [node * dof + d for node in nodes for d in range(dof)]
                rows += [cols] * dof
    case = from_rows(rows)
    assert case.n == nx * ny * nz * dof and np.array_equal(np.flatnonzero(case.nat), np.arange(0, case.n, dof))
    return case


@functools.lru_cache(maxsize=None)
def long_chain_case(chunk, chunks=64):
    """At least ``chunks`` chunks of rows with five entries each, in natural runs of random lengths 1 ... 200."""
    rng = np.random.default_rng(7300)
    lengths = []
    while sum(lengths) < chunks * chunk + 11:
        lengths.append(int(rng.integers(1, 201)))
    case = runs_case(lengths, 7301)
    assert case.n >= chunks * chunk and max(lengths) > 128 and min(lengths) == 1
    return case


@functools.lru_cache(maxsize=None)
def long_chain_want(chunk, max_order, agglomerate):
    case = long_chain_case(chunk)
    return mirror_starts(case.crow, case.col, max_order, agglomerate, case.nat)
