"""The reference and the case generators of the CSR block gather (``Inverter.csr_diag_blocks`` / ``inv_csr_blocks``,
``mi32_csr_blocks_device*``).  No pytest in here: the test files import what they need.

The reference is a NumPy restatement of the contract by ASSIGNMENT, sharing nothing with the kernel:

    per block (first row and column f, order n), per row i:
        m = (col_seg >= f) & (col_seg < f + n)
        out[i, col_seg[m] - f] = val_seg[m]          # on zeros

``mirror_sources`` applies it to the entries' own indices -- which stored entry lands in which output element, -1 for
none -- and ``mirror_blocks`` moves the values' BITS through that map, so a stored -0.0, NaN payload or subnormal is
neither read as a number nor rounded, and the +0.0 of an absent entry is the all-zero word.  (``to_dense()`` is not a
reference: it turns a stored -0.0 into +0.0.)  The map depends on the structure alone, so the tests of one case in
fp32 / fp64 and int32 / int64 share one.

Every generator asserts on the host that its case has the property it is named for.  A case is a namespace of
``n`` (rows), ``crow``, ``col`` (int64), ``val`` (float64 holding float32-representable numbers, so that both element
types see the same matrix), ``orders``, ``first`` (None: consecutive blocks) and whatever the case adds.
"""
import functools
from types import SimpleNamespace

import numpy as np

UINT = {4: np.uint32, 8: np.uint64}
LANE_TOPS = (8, 16, 32, 64, 128)


def lanes_of(n):
    return next(top for top in LANE_TOPS if n <= top)


def consecutive(orders):
    """The first rows of consecutive diagonal blocks: the exclusive prefix sum of the orders."""
    return np.concatenate(([0], np.cumsum(np.asarray(orders, np.int64))[:-1]))


def flat_offsets(orders):
    """Element offset of every block in the packed layout, and the total."""
    off = np.concatenate(([0], np.cumsum(np.asarray(orders, np.int64) ** 2)))
    return off[:-1], int(off[-1])


def mirror_sources(crow, col, orders, first=None):
    """The packed int64 map: for every output element the index into col / val of the entry that is assigned to it,
    -1 where the CSR stores none.  The rule of the module docstring, the rows of a block taken together (each row's
    segment keeps its own row index)."""
    crow, col = np.asarray(crow, np.int64), np.asarray(col, np.int64)
    first = consecutive(orders) if first is None else np.asarray(first, np.int64)
    offs, total = flat_offsets(orders)
    out = np.full(total, -1, np.int64)
    for n, f, o in zip(orders, first, offs):
        n, f = int(n), int(f)
        s, e = crow[f], crow[f + n]
        seg = col[s:e]
        row = np.repeat(np.arange(n), np.diff(crow[f:f + n + 1]))
        m = (seg >= f) & (seg < f + n)
        blk = out[o:o + n * n].reshape(n, n)
        blk[row[m], seg[m] - f] = np.arange(s, e)[m]
    return out


def mirror_blocks(crow, col, val, orders, first=None, sources=None):
    """The packed reference of val's dtype: the bits of the assigned entry, the all-zero word (+0.0) elsewhere."""
    src = mirror_sources(crow, col, orders, first) if sources is None else sources
    bits = np.ascontiguousarray(val).view(UINT[val.dtype.itemsize])
    out = np.zeros(src.size, bits.dtype)
    hit = src >= 0
    out[hit] = bits[src[hit]]
    return out.view(val.dtype)


def same_bytes(got, want, tag=""):
    """Bytes equal, no tolerance; the message names the first element that differs."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.dtype, want.dtype, got.shape, want.shape)
    g, w = got.reshape(-1).view(UINT[got.dtype.itemsize]), want.reshape(-1).view(UINT[want.dtype.itemsize])
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, (tag, f"{bad.size} of {g.size} elements differ, first at {int(bad[0])}: "
                                f"{hex(int(g[bad[0]]))} for {hex(int(w[bad[0]]))}")


def typed(case, vdtype, idtype):
    """(crow, col, val) of a case in the given value and index dtypes.  ``case.bits`` (values' bits per dtype, for the
    cases that store what a cast would not keep) wins over the cast of ``case.val``."""
    bits = getattr(case, "bits", None)
    val = bits[np.dtype(vdtype).itemsize].view(vdtype) if bits else case.val.astype(vdtype)
    return case.crow.astype(idtype), case.col.astype(idtype), val


# ---- building CSR structures ------------------------------------------------------------------------------------------
def csr_from_pairs(n, rows, cols, rng):
    """(crow, col) of the distinct (row, col) pairs, the columns of every row in a random order."""
    key = np.unique(np.asarray(rows, np.int64) * n + np.asarray(cols, np.int64))
    r, c = key // n, key % n
    order = np.lexsort((rng.random(key.size), r))
    r, c = r[order], c[order]
    crow = np.concatenate(([0], np.cumsum(np.bincount(r, minlength=n)))).astype(np.int64)
    assert crow[-1] == c.size and (np.diff(crow) >= 0).all()
    assert no_duplicates(n, crow, c)
    return crow, c


def rows_of_entries(crow):
    return np.repeat(np.arange(crow.size - 1), np.diff(crow))


def no_duplicates(n, crow, col):
    key = rows_of_entries(crow) * n + col
    return np.unique(key).size == key.size


def has_unsorted_row(crow, col):
    inner = np.ones(col.size, bool)
    inner[crow[:-1][np.diff(crow) > 0]] = False        # the first entry of a row has no left neighbour in it
    return bool((np.diff(col, prepend=col[:1])[inner] < 0).any())


def values_for(count, rng):
    """Nonzero float32-representable numbers, all distinct from zero so that an arrival shows."""
    v = rng.uniform(0.5, 2.0, count) * rng.choice([-1.0, 1.0], count)
    return v.astype(np.float32).astype(np.float64)


def inside_fraction(case):
    src = mirror_sources(case.crow, case.col, case.orders, case.first)
    return int((src >= 0).sum()) / max(1, case.col.size)


def _case(n, crow, col, val, orders, first=None, **more):
    orders = np.asarray(orders, np.int32)
    f = consecutive(orders) if first is None else np.asarray(first, np.int64)
    assert (f >= 0).all() and (f + orders <= n).all() and crow.size == n + 1 and col.size == val.size == crow[-1]
    assert first is not None or int(orders.sum()) == n
    return SimpleNamespace(n=n, crow=crow, col=col, val=val, orders=orders, first=first, **more)


# ---- the cases -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def every_order_case(seed=7001):
    """Every order 1 ... 128 once, shuffled, as the consecutive blocks of one matrix of 8256 rows: about 12 random
    entries per row, most of them outside the blocks, and a band of half-width 40 at density 1/2 that reaches into
    every block; columns unsorted.  The orders are the same for every seed, the entries are not."""
    rng = np.random.default_rng(seed)
    orders = np.random.default_rng(7000).permutation(np.arange(1, 129))
    n = int(orders.sum())
    assert n == 8256
    r1 = np.repeat(np.arange(n), 12)
    c1 = rng.integers(0, n, r1.size)
    r2 = np.repeat(np.arange(n), 81)
    c2 = r2 + np.tile(np.arange(-40, 41), n)
    keep = (c2 >= 0) & (c2 < n) & ((rng.random(r2.size) < 0.5) | (c2 == r2))   # (the diagonal always: order 1 has no more)
    crow, col = csr_from_pairs(n, np.concatenate((r1, r2[keep])), np.concatenate((c1, c2[keep])), rng)
    case = _case(n, crow, col, values_for(col.size, rng), orders)
    assert has_unsorted_row(crow, col)
    src = mirror_sources(crow, col, orders)
    offs, _ = flat_offsets(orders)
    assert all((src[o:o + int(k) ** 2] >= 0).any() for k, o in zip(orders, offs))           # the band fills parts of every block
    rnd = np.isin(rows_of_entries(crow) * n + col, r1.astype(np.int64) * n + c1)
    hit = np.zeros(col.size, bool)
    hit[src[src >= 0]] = True
    assert (hit & rnd).sum() < 0.1 * rnd.sum()                                              # most random entries fall outside
    return case


SEAM_ORDERS = (5, 8, 13, 16, 30, 32, 50, 64, 100, 128, 1, 3)


@functools.lru_cache(maxsize=None)
def seams_case():
    """A block of each lane class (and the edges of the classes), the first and the last block of the matrix among
    them: every row of a block holds entries at the columns first - 1 and first + n, one off on either side, and at
    first and first + n - 1.  The inner ones must arrive, the outer ones nowhere.  ``inner``: the entry indices that
    must arrive."""
    rng = np.random.default_rng(7002)
    orders = np.array(SEAM_ORDERS)
    assert {lanes_of(k) for k in orders} == set(LANE_TOPS)
    n = int(orders.sum())
    first = consecutive(orders)
    rows, cols = [], []
    for k, f in zip(orders, first):
        for c in (f - 1, f, f + k - 1, f + k):
            if 0 <= c < n:
                rows.append(np.arange(f, f + k))
                cols.append(np.full(k, c))
    crow, col = csr_from_pairs(n, np.concatenate(rows), np.concatenate(cols), rng)
    case = _case(n, crow, col, values_for(col.size, rng), orders)
    r = rows_of_entries(crow)
    blk = np.searchsorted(first, r, side="right") - 1
    f, k = first[blk], orders[blk]
    inner = (col == f) | (col == f + k - 1)
    outer = (col == f - 1) | (col == f + k)
    assert (inner ^ outer).all() and outer.sum() == 2 * n - orders[0] - orders[-1] and inner.sum() == 2 * n - (orders == 1).sum()
    src = mirror_sources(crow, col, orders)
    assert np.array_equal(np.sort(src[src >= 0]), np.nonzero(inner)[0])
    case.inner = np.nonzero(inner)[0]
    return case


ROW_SHAPE_ORDERS = (6, 12, 24, 48, 96, 128, 128, 128, 128, 128, 2)


@functools.lru_cache(maxsize=None)
def row_shapes_case():
    """Per block of each lane class: row 0 empty, row 1 with 700 entries (every column of the block among them, so
    the scan runs several rounds for every group width), row 2 with entries only outside the block; the other rows
    hold a few entries.  The block of order 128 at index 6 is fully dense."""
    rng = np.random.default_rng(7003)
    orders = np.array(ROW_SHAPE_ORDERS)
    n = int(orders.sum())
    first = consecutive(orders)
    assert n >= 700 and {lanes_of(k) for k in orders[:6]} == set(LANE_TOPS)
    rows, cols = [], []
    for b, (k, f) in enumerate(zip(orders, first)):
        inside = np.arange(f, f + k)
        outside = np.setdiff1d(np.arange(n), inside)
        if b == 6:                                             # fully dense
            rows.append(np.repeat(inside, k))
            cols.append(np.tile(inside, k))
            continue
        for i in range(k):
            if i == 0 and k > 1:
                continue                                       # empty
            if i == 1 and b < 6:
                c = np.concatenate((inside, rng.choice(outside, 700 - k, replace=False)))
            elif i == 2:
                c = rng.choice(outside, 9, replace=False)
            else:
                c = rng.choice(n, 5, replace=False)
            rows.append(np.full(c.size, f + i))
            cols.append(c)
    crow, col = csr_from_pairs(n, np.concatenate(rows), np.concatenate(cols), rng)
    case = _case(n, crow, col, values_for(col.size, rng), orders)
    length = np.diff(crow)
    src = mirror_sources(crow, col, orders)
    offs, _ = flat_offsets(orders)
    for b, (k, f, o) in enumerate(zip(orders, first, offs)):
        blk = src[o:o + k * k].reshape(k, k)
        if b == 6:
            assert (blk >= 0).all()
            continue
        if k > 1:
            assert length[f] == 0
        if b < 6:
            assert length[f + 1] == 700 and (blk[1] >= 0).all()
        if k > 2:
            assert length[f + 2] == 9 and (blk[2] < 0).all()
    assert has_unsorted_row(crow, col)
    return case


def special_bits(size):
    """The words of the stored values that must arrive bit for bit: zeros of both signs, quiet and signalling NaNs with
    payloads and both signs, infinities, the smallest and the largest subnormal of both signs."""
    if size == 4:
        w = [0x80000000, 0x00000000, 0x7FC00000, 0xFFC12345, 0x7F800001, 0xFFA00000, 0x7F800000, 0xFF800000,
             0x00000001, 0x807FFFFF, 0x00400000, 0x80000001]
    else:
        w = [0x8000000000000000, 0x0, 0x7FF8000000000000, 0xFFF8123456789ABC, 0x7FF0000000000001, 0xFFF4000000000000,
             0x7FF0000000000000, 0xFFF0000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x0008000000000000,
             0x8000000000000001]
    return np.array(w, UINT[size])


VALUE_ORDERS = (7, 14, 29, 60, 115, 4)


@functools.lru_cache(maxsize=None)
def values_case():
    """Blocks of every lane class, fully stored, whose entries cycle through ``special_bits`` (ordinary numbers between
    them); off-block entries hold specials too and must not arrive.  ``bits``: the stored words per element size."""
    rng = np.random.default_rng(7004)
    orders = np.array(VALUE_ORDERS)
    n = int(orders.sum())
    first = consecutive(orders)
    rows = np.concatenate([np.repeat(np.arange(f, f + k), k) for k, f in zip(orders, first)] + [np.arange(n)])
    cols = np.concatenate([np.tile(np.arange(f, f + k), k) for k, f in zip(orders, first)] + [rng.integers(0, n, n)])
    crow, col = csr_from_pairs(n, rows, cols, rng)
    val = values_for(col.size, rng)
    bits = {}
    for size, ftype in ((4, np.float32), (8, np.float64)):
        b = val.astype(ftype).view(UINT[size]).copy()
        sp = special_bits(size)
        at = np.arange(0, col.size, 2)                         # every other entry is a special one
        b[at] = sp[(at // 2) % sp.size]
        bits[size] = b
    case = _case(n, crow, col, val, orders, bits=bits)
    src = mirror_sources(crow, col, orders)
    assert (src >= 0).all()                                    # fully stored blocks
    for size in (4, 8):                                        # every special word sits inside a block
        assert set(special_bits(size).tolist()) <= set(bits[size][src].tolist())
    return case


@functools.lru_cache(maxsize=None)
def first_rows_case():
    """Blocks given by ``first``: overlapping ones (two at the same row, one inside another, two that share rows), gaps
    of rows that belong to no block, and blocks at row 0 and at the last row."""
    rng = np.random.default_rng(7006)
    n = 600
    orders = np.array([8, 16, 5, 64, 128, 30, 128, 1, 70])
    first = np.array([0, 3, 3, 100, 90, 400, n - 128, 250, 455])
    r = np.repeat(np.arange(n), 40)
    c = np.clip(r + rng.integers(-90, 91, r.size), 0, n - 1)
    crow, col = csr_from_pairs(n, r, c, rng)
    case = _case(n, crow, col, values_for(col.size, rng), orders, first)
    covered = np.zeros(n, np.int32)
    for k, f in zip(orders, first):
        covered[f:f + k] += 1
    assert (covered == 0).any() and (covered >= 2).any() and (covered == 3).any() and covered[0] and covered[-1]
    assert {lanes_of(k) for k in orders} == set(LANE_TOPS)
    return case


@functools.lru_cache(maxsize=None)
def many_members_case():
    """70 000 consecutive blocks of orders 1 ... 8 (one lane class): about 315 000 rows at about 10 entries per row
    around the diagonal.  ``sources``: the reference map, computed once for every dtype."""
    rng = np.random.default_rng(7007)
    orders = rng.integers(1, 9, 70_000)
    n = int(orders.sum())
    assert 300_000 < n < 330_000
    r = np.repeat(np.arange(n), 11)
    c = np.clip(r + rng.integers(-12, 13, r.size), 0, n - 1)
    crow, col = csr_from_pairs(n, r, c, rng)
    assert 8.5 < col.size / n < 11
    case = _case(n, crow, col, values_for(col.size, rng), orders)
    case.sources = mirror_sources(crow, col, orders)
    assert (case.sources >= 0).sum() > n                       # the blocks are not empty
    return case


def block_jacobi_case(orders, seed=7008, singular=None):
    """The project's own example as a sparse matrix: every diagonal block fully stored, U(-1, 1) + sqrt(n) I, and three
    entries per row outside the blocks; ``singular``: the block whose row 0 stores nothing inside the block, so that it
    is exactly singular.  ``dense``: the same matrix as a dense float32 array (zeros where nothing is stored)."""
    rng = np.random.default_rng(seed)
    orders = np.asarray(orders)
    n = int(orders.sum())
    first = consecutive(orders)
    dense = np.zeros((n, n), np.float32)
    r = np.repeat(np.arange(n), 3)
    c = rng.integers(0, n, r.size)
    dense[r, c] = values_for(r.size, rng)
    for b, (k, f) in enumerate(zip(orders, first)):
        dense[f:f + k, f:f + k] = rng.uniform(-1, 1, (k, k)) + np.sqrt(k) * np.eye(k)
        if b == singular:
            dense[f, f:f + k] = 0
    rows, cols = np.nonzero(dense)
    crow, col = csr_from_pairs(n, rows, cols, rng)
    val = dense[rows_of_entries(crow), col].astype(np.float64)
    assert (val != 0).all()
    return _case(n, crow, col, val, orders, dense=dense)
