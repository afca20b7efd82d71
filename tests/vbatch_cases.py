"""Inputs and helpers of the variable-size batch tests (tests/test_gpu_vbatch.py, tests/test_vbatch_abi.py).  The
matrix families are those of tests/resident_cases.py."""
import numpy as np

from conftest import gate_matrix
from resident_cases import dist_matrix, dominant

KINDS = ("gate", "ref100", "rand", "hollow")
CLASS_TOPS = (8, 16, 32, 64, 80, 96, 112, 128)   # the largest order each of the eight kernel classes takes
BIG_MEMBERS = 70_000
# the shapes tools/mixed_batch_bench.py measures: (members, lowest order, highest order); the test asserts the first two
BENCH_SHAPES = [(16_384, 3, 64), (4_096, 65, 128), (65_536, 1, 128)]


def class_begin(orders):
    """What mi32_vbatch_bin answers for the class ranges: the counts at the boundaries 8 / 16 / ... / 128."""
    o = np.asarray(orders)
    return [0] + [int((o <= top).sum()) for top in CLASS_TOPS]


def every_order_members():
    """511 members: every order 1 ... 128 in every family (hollow needs two rows), shuffled."""
    mats = [dist_matrix(KINDS[k], n, 29_000 + 100 * n + k)
            for n in range(1, 129) for k in range(len(KINDS)) if not (KINDS[k] == "hollow" and n == 1)]
    assert len(mats) == 511
    return [mats[i] for i in np.random.default_rng(1).permutation(len(mats))]


def dominant_members(dtype):
    """One strictly diagonally dominant member per order 1 ... 128, shuffled: the no-pivot variant's inputs."""
    mats = [dominant(n, 800 + n, dtype) for n in range(1, 129)]
    return [mats[i] for i in np.random.default_rng(1).permutation(len(mats))]


def big_mixed_members():
    """70 000 well-conditioned, row-permuted members of orders 1 ... 12, drawn in member order from ONE generator."""
    rng = np.random.default_rng(6100)
    orders = rng.integers(1, 13, BIG_MEMBERS)
    return [(rng.uniform(-1, 1, (n, n)) + np.sqrt(n) * np.eye(n))[rng.permutation(n)].astype(np.float32)
            for n in orders]


def invalid_between_valid():
    """Orders [20, 5, 20, 31, 17, 20, 100, 9, 100].  Sorted by order the register-resident classes take 5, 9 | 17, 20,
    20, 20, 31 -- the 32-lane class holds two members per wave, so the wave (17, 20) holds the rank-1 member 0 beside
    the valid member 4 of another order, and the wave (20, 20) the NaN member 2 beside the valid member 5; the all-zero
    member 8 sits beside the valid member 6 in the workgroup class.  Returns (members, expected statuses)."""
    orders = [20, 5, 20, 31, 17, 20, 100, 9, 100]
    mats = [gate_matrix(n, 7700 + b) for b, n in enumerate(orders)]
    mats[0][:] = 1.0
    mats[2][4, 7] = np.nan
    mats[8][:] = 0.0
    return mats, [2, 0, 2, 0, 0, 0, 0, 0, 2]


def diag_block_orders(total=3000):
    """Block orders 1 ... 128 from default_rng(6) that sum to `total` (the last one is cut to fit)."""
    rng = np.random.default_rng(6)
    orders = []
    while sum(orders) < total:
        orders.append(int(min(rng.integers(1, 129), total - sum(orders))))
    return orders


def bench_members(members, lo, hi, dtype=np.float32, dominant_rows=False, seed=0):
    """(orders, packed flat array) of `members` members with orders uniform in lo ... hi; U(-1, 1) + sqrt(n) I, or
    strictly diagonally dominant for the no-pivot variant.  The orders depend on the shape alone; the entries are
    drawn order by order from a generator that `seed` selects, so two seeds give two data sets for one plan."""
    orders = np.random.default_rng(9900 + members % 997 + hi).integers(lo, hi + 1, members)
    rng = np.random.default_rng([9900 + members % 997 + hi, seed])
    flat = np.empty(int((orders.astype(np.int64) ** 2).sum()), dtype)
    off = np.concatenate(([0], np.cumsum(orders.astype(np.int64) ** 2)))
    for n in np.unique(orders):
        idx = np.nonzero(orders == n)[0]
        a = rng.uniform(-1, 1, (idx.size, n, n))
        if dominant_rows:
            a[:, np.arange(n), np.arange(n)] = np.abs(a).sum(axis=2) + 1.0
        else:
            a += np.sqrt(n) * np.eye(n)
        a = a.astype(dtype).reshape(idx.size, n * n)
        for k, b in enumerate(idx):
            flat[off[b]:off[b + 1]] = a[k]
    return orders, flat


def pack(mats):
    """(orders, flat): the packed layout, member b at offset sum_{i<b} n_i^2."""
    orders = np.array([m.shape[0] for m in mats], np.int32)
    return orders, np.concatenate([np.ascontiguousarray(m).reshape(-1) for m in mats])


def unpack(flat, orders):
    off = np.concatenate(([0], np.cumsum(np.asarray(orders, np.int64) ** 2)))
    return [flat[off[b]:off[b + 1]].reshape(int(n), int(n)) for b, n in enumerate(orders)]


def oracle_members(fn, mats):
    """(inverses, statuses) of the CPU oracle function `fn(vec, n, return_info=True)` member by member."""
    outs, st = [], []
    for m in mats:
        n = m.shape[0]
        x, info = fn(m, n, return_info=True)
        outs.append(np.asarray(x).reshape(n, n) if np.asarray(x).size == n * n else None)
        st.append(int(info["status"]))
    return outs, st
