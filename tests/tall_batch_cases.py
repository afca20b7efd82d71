"""Batches of the blocked fp32 path above 4096 padded rows (tests/test_tall_batch_cases.py proves the cases on the CPU
oracle and pins the plans, tests/test_gpu_tall_batches.py runs them on the GPU).  Pure numpy, seeded.

Above 4096 padded rows the host takes another route for every batch size ("Routing above 4096
rows"): shared panels with a batch index (batch 2 ... 4), one 1024-thread workgroup with 8 or 16 rows per lane and
the batch split over two streams (batch >= 5), block width 128 (batch >= 8).  A member of such a batch needs a known
answer, and the oracle takes seconds per matrix at these orders.  So a batch holds TWO independent base matrices, each
checked against the oracle itself, and exact transforms of them, whose inverse follows from the base's bit for bit:

  * with pivoting, ``variant``: a1 = 2^k P a D (P a row permutation, D = diag(+-1)).  Partial pivoting picks the same
    rows by value, sign flips and power-of-two scalings are exact, so inv(a1) = 2^-k D inv(a) P^T in every bit.  The
    permutation puts a member's winning rows into other workgroups of a shared panel than its base's at the same step.
  * without pivoting, ``variant_nopivot``: a1 = D1 a D2 with diagonal entries +-2^e: inv(a1) = D2^-1 inv(a) D1^-1.

No tolerance anywhere: everything here is compared as bytes (conftest.canonical_bytes: -0.0 stored as +0.0, which a
sign flip of a zero produces).
"""
import collections

import numpy as np

from conftest import gate_matrix

N_TALL = 4200    # 4224 padded rows: two workgroups per shared panel; 8 rows per lane where one workgroup holds them
N_WIDE = 8200    # 8320 padded rows: three workgroups per shared panel; 16 rows per lane
SEED_GATE = 40_000   # gate_matrix(4200, 40_000) is the single matrix of the shared-panel tests in test_gpu_parity.py
SEED_REF = 40_100
K_FULL_DIVISION = 40   # 2^40 x the entries puts the pivot rows' processed columns below 2^-47: full division (mi32_strip.h)
# exponents of a batch's third, fourth, ... member: exactly one K_FULL_DIVISION per batch
VARIANT_KS = (K_FULL_DIVISION, -9, 3, -9, 3, -30)

PivotTransform = collections.namedtuple("PivotTransform", "perm d k")
NoPivotTransform = collections.namedtuple("NoPivotTransform", "d1 d2")
# matrix; key of its base in the oracle cache, (kind, n, seed); None for a base itself, else the transform
Member = collections.namedtuple("Member", "matrix base transform")


def base_member(kind, n, seed):
    """"gate": conftest.gate_matrix; "ref100": U(0, 100), the reference's own input distribution, as dist_matrix of
    tests/test_gpu_parity.py draws it."""
    if kind == "gate":
        return gate_matrix(n, seed)
    if kind == "ref100":
        return np.random.default_rng(seed).uniform(0, 100, (n, n)).astype(np.float32)
    raise ValueError(kind)


def dominant(n, seed):
    """Strictly diagonally dominant fp32 matrix (no pivoting needed), as _dominant of tests/test_gpu_parity.py."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, (n, n))
    a[np.arange(n), np.arange(n)] = np.abs(a).sum(axis=1) + 1.0
    return a.astype(np.float32)


def variant(a, seed, k):
    """(a1, transform): a1 = 2^k P a D with P, D drawn from default_rng([seed, n]); see ``apply_variant``."""
    n = a.shape[0]
    assert a.dtype == np.float32 and a.shape == (n, n)
    rng = np.random.default_rng([seed, n])
    perm = rng.permutation(n)
    d = rng.choice(np.array([-1.0, 1.0], np.float32), n)
    a1 = np.ascontiguousarray((a[perm] * d[None, :]) * np.float32(2.0) ** k)
    assert a1.dtype == np.float32 and np.isfinite(a1).all()
    assert np.array_equal(np.abs(a1) * np.float32(2.0) ** -k, np.abs(a[perm]))   # nothing was rounded
    return a1, PivotTransform(perm, d, k)


def apply_variant(x, t):
    """inv(a1) from x = inv(a), both (n, n): the sign flip of the rows, the column gather, the division by 2^k -- in
    that order, all exact in fp32 (the GPU test does the same three steps on the device)."""
    n = t.perm.size
    x = np.asarray(x, np.float32).reshape(n, n)
    return (x * t.d[:, None])[:, t.perm] / np.float32(2.0) ** t.k


def variant_nopivot(a, seed):
    """(a1, transform): a1 = D1 a D2, the diagonals +-2^e with e in -8 ... 8 from default_rng([seed, n])."""
    n = a.shape[0]
    assert a.dtype == np.float32 and a.shape == (n, n)
    rng = np.random.default_rng([seed, n])
    d1, d2 = (np.ldexp(rng.choice([-1.0, 1.0], n), rng.integers(-8, 9, n)).astype(np.float32) for _ in range(2))
    a1 = np.ascontiguousarray(d1[:, None] * a * d2[None, :])
    assert a1.dtype == np.float32 and np.isfinite(a1).all()
    return a1, NoPivotTransform(d1, d2)


def apply_variant_nopivot(x, t):
    n = t.d1.size
    x = np.asarray(x, np.float32).reshape(n, n)
    return x / t.d2[:, None] / t.d1[None, :]


# ---- the batches -----------------------------------------------------------------------------------------------------
_BASES = {}      # (kind, n, seed) -> matrix
_INVERSES = {}   # (kind, n, seed) -> the oracle's flat inverse: batches of 2, 3, 4, 5 and 8 share two oracle runs


def cached_base(kind, n, seed):
    key = (kind, n, seed)
    if key not in _BASES:
        a = base_member(kind, n, seed)
        a.setflags(write=False)
        _BASES[key] = a
    return _BASES[key]


def oracle_inverse(oracle, key):
    """The reference-order result on the base ``key``: the step-by-step restatement up to N = 1024, above that its
    block-by-block evaluation (tests/test_oracle.py proves the two bit-identical for every block width).  Run once."""
    if key not in _INVERSES:
        kind, n, seed = key
        fn = oracle.matrix_inv_32_inplace if n <= 1024 else (lambda a, m, **kw: oracle.matrix_inv_32_blocked_exact(a, m, 128, **kw))
        x, info = fn(cached_base(*key), n, return_info=True)
        assert info["status"] == 0, key
        x.setflags(write=False)
        _INVERSES[key] = x
    return _INVERSES[key]


def tall_batch(n, batch, rotate=0):
    """``batch`` Members of order n: a gate base, a ref100 base, then variants of the two in turn, each with a
    permutation of its own and the exponents VARIANT_KS.  ``rotate`` starts the list that many members later (cyclic
    over the first eight), so that a batch of two can hold a variant too: rotate=1 is [ref100 base, 2^40 gate variant]."""
    assert 1 <= batch <= 8 and 0 <= rotate < 8
    keys = (("gate", n, SEED_GATE), ("ref100", n, SEED_REF))
    members = []
    for i in range(rotate, rotate + batch):
        i %= 8
        key = keys[i % 2]
        if i < 2:
            members.append(Member(cached_base(*key), key, None))
        else:
            a1, t = variant(cached_base(*key), 1000 + i, VARIANT_KS[i - 2])
            members.append(Member(a1, key, t))
    return members


def expected_inverse(oracle, member):
    """The (n, n) inverse the oracle gives for a Member: its own run for a base, the exact transform of it otherwise."""
    x = oracle_inverse(oracle, member.base)
    n = member.matrix.shape[0]
    return x.reshape(n, n) if member.transform is None else apply_variant(x, member.transform)


# ---- the plans the GPU tests rely on (mi32_resolve_blocking / mi32_resolve_panel_widths) --------------------------
# (n, batch, MI32_MULTI_PANEL or None, block width, sub-panel width of every block)
PLANS = [
    (N_TALL, 1, None, 256, [16] * 17),
    (N_TALL, 2, None, 256, [16] * 17),
    (N_TALL, 3, None, 256, [16] * 17),
    (N_TALL, 4, None, 256, [16] * 17),             # 4 x kMaxPanelGroups = 16: the largest batch with shared panels
    (N_TALL, 5, None, 256, [8] + [16] * 16),       # one workgroup, 8 rows per lane: W = 8 while > 4096 rows are candidates
    (N_TALL, 8, None, 128, [8] + [16] * 32),       # >= 8 matrices and >= 64 Mi elements: block width 128
    (N_WIDE, 1, "0", 256, [4] + [8] * 16 + [16] * 16),   # 16 rows per lane: W = 4; 8 rows per lane down to 4224 rows
    (N_WIDE, 2, None, 256, [16] * 33),
    (N_WIDE, 5, None, 256, [4] + [8] * 16 + [16] * 16),  # what the single-matrix case above stands in for
]
