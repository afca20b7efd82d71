"""Inputs and helpers of the wide workgroup-resident path's tests (tests/test_gpu_wide.py, tests/test_wide_abi.py,
tests/test_wide_code_object.py).  The matrix families are those of tests/resident_cases.py; the degenerate, subnormal
and overflowing inputs come from the generators of their own modules, at this path's orders."""
import numpy as np

import overflow_cases as ovf
import subnormal_cases as sub
from conftest import gate_matrix
from degenerate_cases import duplicate_rows, zero_column
from resident_cases import dist_matrix, dominant, oracle_batch, run, tie_batch  # noqa: F401
from workgroup_cases import anti_diagonal, mixed_batch, slot_batch, zero_diagonal_entry  # noqa: F401

KINDS = ("gate", "ref100", "rand", "hollow")
ORDERS = list(range(129, 257))
# both ends of every class (160 / 192 / 224 / 256 padded rows): 129 leaves 63 of 192 column lanes idle, 192 and 256 none
EDGE_ORDERS = [129, 160, 161, 192, 193, 224, 225, 256]
TIE_ORDERS = [129, 192, 256]
SLOT_ORDERS = [129, 193, 256]
DET_ORDERS = [129, 192, 193, 256]
EXTREME_ORDERS = [129, 256]
MEMBERS = 3
MAX_ORDER = 256
BIG_ORDER, BIG_BATCH, BIG_DISTINCT = 129, 66_000, 256
# The shapes whose direction tests/test_gpu_wide.py asserts.  (256, 1024) was on this list and left it: on an MI355X the
# wide path loses there (3.29 ms against the blocked path's 2.67 ms: an order-256 batch is the one shape the blocked
# path neither pads nor splits); tools/wide_batch_bench.py still measures it and the README table reports the loss.
TIMED_SHAPES = [(160, 2_048)]


def wide_class(n):
    """(threads per matrix, register rows per thread) of the class that takes order n; (0, 0) outside 129 ... 256."""
    if not 129 <= n <= 256:
        return 0, 0
    return (768, 40) if n <= 160 else (768, 48) if n <= 192 else (1024, 56) if n <= 224 else (1024, 64)


# (columns per slab, rows per thread) of the four classes
CLASSES = [(192, 40), (192, 48), (256, 56), (256, 64)]


def family_batch(kind, n, members=MEMBERS):
    return np.stack([dist_matrix(kind, n, 19_000 + 100 * n + b) for b in range(members)])


def dominant_batch(n, dtype=np.float32, members=MEMBERS):
    return np.stack([dominant(n, 700 + n + b, dtype) for b in range(members)])


def late_singular_batch(n):
    """gate, gate with its LAST column zero (the bad pivot is met at step n - 1), gate, gate with the last row equal
    to the first (status 0, a huge inverse), gate."""
    return np.stack([gate_matrix(n, 4400 + n), zero_column(n, n - 1, 4401 + n), gate_matrix(n, 4402 + n),
                     duplicate_rows(n, 4403 + n), gate_matrix(n, 4404 + n)])


def nan_in_last_slab():
    """Three matrices of order 256; member 1 holds a NaN in row 250: register slot 58 of the fourth slab."""
    mats = np.stack([gate_matrix(256, 4500 + b) for b in range(3)])
    mats[1, 250, 7] = np.nan
    return mats


def subnormal_batch(n, pivoting):
    """One input per recipe of subnormal_cases at order n: (batch, family names)."""
    names = sub.PIVOTED if pivoting else sub.NOPIVOT
    return np.stack([sub.matrix(f, n, np.float32) for f in names]), names


def overflow_out(n):
    """subnormal_cases.overflow_out's recipe at order n: gate_matrix(n, 5000 + n) * 2^-130."""
    return sub.scaled(gate_matrix(n, 5000 + n), -130, np.float32)


def overflow_batch(n, pivoting):
    """One input per recipe of overflow_cases at order n (rows_down, block_diag with three quarters of the order in
    the overflowing block, which comes first): (batch, cases)."""
    cs = [c for c in ovf.one_launch_cases(n, np.float32, pivoting) if c.kind != "plain"]
    return np.stack([ovf.matrix(c) for c in cs]), cs


def big_distinct():
    """BIG_DISTINCT well-conditioned, row-permuted matrices of order BIG_ORDER from ONE generator."""
    n = BIG_ORDER
    rng = np.random.default_rng(5100 + n)
    a = rng.uniform(-1, 1, (BIG_DISTINCT, n, n)) + np.sqrt(n) * np.eye(n)
    perm = rng.permuted(np.tile(np.arange(n), (BIG_DISTINCT, 1)), axis=1)
    return np.take_along_axis(a, perm[:, :, None], axis=1).astype(np.float32)


def big_index():
    """Which of the distinct matrices each of the BIG_BATCH members is: every one of them, in a shuffled order."""
    rng = np.random.default_rng(5300)
    return np.concatenate([rng.permutation(BIG_DISTINCT) for _ in range(-(-BIG_BATCH // BIG_DISTINCT))])[:BIG_BATCH]
