"""Inputs and helpers of the workgroup-resident path's tests (tests/test_gpu_workgroup.py).  The matrix families are
those of tests/resident_cases.py."""
import numpy as np

from conftest import gate_matrix
from degenerate_cases import signed_pow2_permutation
from resident_cases import dist_matrix, dominant, oracle_batch, run, tie_batch  # noqa: F401

KINDS = ("gate", "ref100", "rand", "hollow")
ORDERS = list(range(65, 129))
# both ends of every rows-per-thread instance (80 / 96 / 112 / 128 padded rows) and two orders inside
FP64_ORDERS = [65, 72, 80, 81, 96, 97, 112, 113, 127, 128]
TIE_ORDERS = [72, 96, 128]
# the first and the last order of every rows-per-thread instance; 81 and 113 pad to 96 and 128 rows of which the second
# 64-slot label register holds 32 (80 and 112 padded rows are no multiple of 64 either)
SLOT_ORDERS = [65, 80, 81, 96, 112, 113, 128]
MEMBERS = 5
BIG_ORDER, BIG_BATCH, BIG_DISTINCT = 65, 66_000, 256
# the two shapes whose direction tests/test_gpu_workgroup.py asserts
TIMED_SHAPES = [(65, 4_096), (96, 2_048)]


def family_batch(kind, n, members=MEMBERS):
    return np.stack([dist_matrix(kind, n, 19_000 + 100 * n + b) for b in range(members)])


def dominant_batch(n, dtype, members=MEMBERS):
    return np.stack([dominant(n, 700 + n + b, dtype) for b in range(members)])


def zero_diagonal_entry(n, dtype):
    """A dominant matrix whose (1,1) entry is, and stays, exactly zero: the no-pivot variant must report it."""
    h = dominant(n, 700 + n, dtype)
    h[1, 1] = 0.0
    h[1, 0] = 0.0
    return h


def anti_diagonal(n, dtype=np.float32):
    """The exchange matrix: the pivot of step r is the 1 of row n - 1 - r, which never leaves register slot n - 1 - r
    (rows are relabelled, not moved), so the n steps visit every slot of every slab and every label register."""
    return np.ascontiguousarray(np.eye(n, dtype=dtype)[::-1])


def slot_batch(n, dtype=np.float32):
    """(batch, exact inverses): a signed power-of-two permutation matrix and the anti-diagonal one; both inverses are
    known in closed form.  Shared with the wide path's tests (tests/wide_cases.py)."""
    a, x = signed_pow2_permutation(n, 4300 + n, dtype)
    j = anti_diagonal(n, dtype)
    return np.stack([a, j]), np.stack([x, j])


def slot_batch_of_three(n, dtype):
    """slot_batch with a dense third member behind the two permutations: (batch, exact inverses of members 0 and 1)."""
    mats, exact = slot_batch(n, dtype)
    return np.concatenate([mats, gate_matrix(n, 4350 + n).astype(dtype)[None]]), exact


def mixed_batch(n=100):
    """7 matrices of order n: member 2 rank 1, member 4 with a NaN, member 6 all zero, valid ones between them."""
    mats = np.stack([gate_matrix(n, 2600 + b) for b in range(7)])
    mats[2] = 1.0
    mats[4, 70, 3] = np.nan
    mats[6] = 0.0
    return mats, [0, 0, 2, 0, 2, 0, 2]


def big_distinct():
    """BIG_DISTINCT well-conditioned, row-permuted matrices of order BIG_ORDER from ONE generator."""
    n = BIG_ORDER
    rng = np.random.default_rng(5100 + n)
    a = rng.uniform(-1, 1, (BIG_DISTINCT, n, n)) + np.sqrt(n) * np.eye(n)
    perm = rng.permuted(np.tile(np.arange(n), (BIG_DISTINCT, 1)), axis=1)
    return np.take_along_axis(a, perm[:, :, None], axis=1).astype(np.float32)


def big_index():
    """Which of the distinct matrices each of the BIG_BATCH members is: every one of them, in a shuffled order."""
    rng = np.random.default_rng(5200)
    idx = np.concatenate([rng.permutation(BIG_DISTINCT) for _ in range(-(-BIG_BATCH // BIG_DISTINCT))])[:BIG_BATCH]
    return idx
