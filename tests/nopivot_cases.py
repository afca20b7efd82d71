"""Inputs of the no-pivot variant that are NOT diagonally dominant (tests/test_nopivot_cases.py proves them on the CPU
oracle, tests/test_gpu_nopivot.py runs them on every no-pivot GPU path).  Pure numpy, seeded; every generator takes the
dtype.

Elimination without pivoting is stable on a symmetric positive definite matrix whatever its rows look like, so the
valid families are SPD, or exact scalings / sign changes of one:

  * ``spd``: G G^T / n + 0.05 I with G ~ U(-1, 1).  No row is dominant from n = 513 on; kappa_2 about 27;
  * ``spd_scaled``: D spd D with D = diag(2^e), e uniform in [-30, 30] (fp32) or [-250, 250] (fp64): multipliers and
    pivots far from 1 in both directions, a good part of the diagonal outside [2^-47, 2^48).  The scaling is exact, so
    inv(D a D) = D^-1 inv(a) D^-1 bit for bit;
  * ``spd_signed``: spd with a seeded half of its rows negated: about half of the pivots are negative; the inverse is
    spd's with those columns negated, bit for bit;
  * ``sparse_spd``: G G^T with G 2 % dense, plus diag(0.25 * row sum of |.| + 0.01): exact-zero multipliers at every
    step (about two thirds of the entries are exact zeros at n = 1000), not dominant from n = 513 on;
  * ``tridiagonal``: [-1, 2, -1]: weakly dominant only, every multiplier exactly 0 or +-(k / (k + 1)).

Two more are made from a base matrix:

  * ``zero_pivot_at(base, k)``: row k and column k zeroed: the diagonal entry is, and stays, exactly 0 until step k;
  * ``near_cancellation(base, k)``: row k + 1 := row k: the two rows stay equal bit for bit up to step k, whose
    rounding leaves a tiny non-zero pivot for step k + 1.  Status 0 and a huge finite inverse; nothing but its bits
    and the status is asserted.
"""
import functools

import numpy as np

STATUS_OK = 0
STATUS_SINGULAR = 2
FAMILIES = ("spd", "spd_scaled", "spd_signed", "sparse_spd", "tridiagonal")
# the range in which the fp32 strip's shortened division equals the full expansion (mi32_strip.h)
DIV_LO, DIV_HI = 2.0 ** -47, 2.0 ** 48


def spd(n, seed, dtype=np.float32):
    g = np.random.default_rng([seed, n]).uniform(-1.0, 1.0, (n, n))
    return (g @ g.T / n + 0.05 * np.eye(n)).astype(dtype)


def scale_exponents(n, seed, dtype=np.float32):
    """The exponents e of spd_scaled's D = diag(2^e)."""
    top = 30 if np.dtype(dtype) == np.float32 else 250
    return np.random.default_rng([seed, n, 1]).integers(-top, top + 1, n)


def spd_scaled(n, seed, dtype=np.float32):
    d = np.ldexp(1.0, scale_exponents(n, seed, dtype)).astype(dtype)
    a = spd(n, seed, dtype)
    return d[:, None] * a * d[None, :]          # products with powers of two: exact, the order does not matter


def unscale(x, n, seed, dtype):
    """D x D for the D of spd_scaled(n, seed, dtype): maps inv(D a D) back to inv(a), exactly."""
    d = np.ldexp(1.0, scale_exponents(n, seed, dtype)).astype(dtype)
    return d[:, None] * np.asarray(x).reshape(n, n) * d[None, :]


def negated_rows(n, seed):
    """The rows spd_signed negates: a seeded coin per row, so their number is even at one order and odd at another."""
    return np.nonzero(np.random.default_rng([seed, n, 2]).random(n) < 0.5)[0]


def spd_signed(n, seed, dtype=np.float32):
    a = spd(n, seed, dtype)
    a[negated_rows(n, seed)] *= -1
    return a


def sparse_spd(n, seed, dtype=np.float32):
    rng = np.random.default_rng([seed, n, 3])
    g = rng.uniform(-1.0, 1.0, (n, n))
    g[rng.random((n, n)) >= 0.02] = 0.0
    a = g @ g.T
    return (a + np.diag(0.25 * np.abs(a).sum(axis=1) + 0.01)).astype(dtype)


def tridiagonal(n, dtype=np.float32):
    return (2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)).astype(dtype)


def zero_pivot_at(base, k):
    a = np.array(base)
    a[k, :] = 0
    a[:, k] = 0
    return a


def near_cancellation(base, k):
    a = np.array(base)
    a[k + 1] = a[k]
    return a


def seed_of(n):
    """One seed rule for every module that uses these families."""
    return 40_000 + n


@functools.lru_cache(maxsize=None)
def family(name, n, dtype):
    """The member of ``FAMILIES`` at order n in np.float32 / np.float64, computed once per process; read-only."""
    if name == "tridiagonal":
        a = tridiagonal(n, dtype)
    else:
        a = {"spd": spd, "spd_scaled": spd_scaled, "spd_signed": spd_signed, "sparse_spd": sparse_spd}[name](
            n, seed_of(n), dtype)
    a.setflags(write=False)
    return a


# ---- what the families claim, as numbers ----------------------------------------------------------------------------
def dominant_share(a):
    """The share of rows with |a_ii| > sum_{j != i} |a_ij|."""
    m = np.abs(np.asarray(a, np.float64))
    d = np.diag(m)
    return float((d > m.sum(axis=1) - d).mean())


def weakly_dominant_share(a):
    m = np.abs(np.asarray(a, np.float64))
    d = np.diag(m)
    return float((d >= m.sum(axis=1) - d).mean())


def exact_zeros(a):
    return int((np.asarray(a) == 0).sum())


def diagonal_outside_division_range(a):
    d = np.abs(np.diag(np.asarray(a, np.float64)))
    return int(((d < DIV_LO) | (d >= DIV_HI)).sum())


def negative_diagonal(a):
    return int((np.diag(a) < 0).sum())


# ---- the orders and bad-pivot positions the GPU tests use -----------------------------------------------------------
BLOCKED32_ORDERS = (512, 513, 1000)
BLOCKED32_EXPLICIT_ORDERS = (100, 257)
BLOCKED32_WIDTHS = (128, 256, 384, 512)
LOOKAHEAD_ORDER = 2048
BLOCKED64_ORDERS = (512, 513, 640, 1000)
BLOCKED64_EXPLICIT_ORDERS = (65, 257)
BLOCKED64_WIDTHS = (64, 128)
SWEEP_ORDERS = (5, 64, 257, 511)
RESIDENT_ORDERS = (3, 8, 9, 17, 33, 64)
WORKGROUP_ORDERS = (65, 81, 128)
BATCH_ORDER = 600
BATCH_ZERO_STEP = 599
BATCH_CANCEL_STEP = 300
HOST_ORDERS = (513, 640)
ALL_ORDERS = tuple(sorted(set(BLOCKED32_ORDERS + BLOCKED32_EXPLICIT_ORDERS + BLOCKED64_ORDERS + BLOCKED64_EXPLICIT_ORDERS
                              + SWEEP_ORDERS + RESIDENT_ORDERS + WORKGROUP_ORDERS + HOST_ORDERS + (BATCH_ORDER,))))

# (path, dtype, n, block width or 0, steps k): where zero_pivot_at(spd, k) is tried
ZERO_PIVOTS = [
    ("blocked32", np.float32, 1000, 0, (15, 16, 255, 256, 999)),
    ("blocked32", np.float32, 513, 0, (511, 512)),
    ("blocked64", np.float64, 1000, 64, (63, 64, 999)),
    ("blocked64", np.float64, 1000, 128, (127, 128)),
    ("blocked64", np.float64, 513, 0, (512,)),
    # an order that is a multiple of the block width has no padded step: its last step is the last step of the last
    # (sub-panel and) block, and no later step meets the NaNs of a missed zero pivot and flags the member in its place
    ("blocked32", np.float32, 512, 0, (511,)),
    ("blocked64", np.float64, 640, 64, (639,)),
    ("blocked64", np.float64, 640, 128, (639,)),
]
ZERO_PIVOTS += [("sweep", dt, n, 0, (0, n - 1)) for dt in (np.float32, np.float64) for n in SWEEP_ORDERS]
ZERO_PIVOTS += [("resident", dt, n, 0, (0, n - 1)) for dt in (np.float32, np.float64) for n in RESIDENT_ORDERS]
ZERO_PIVOTS += [("workgroup", dt, n, 0, (0, n - 1)) for dt in (np.float32, np.float64) for n in WORKGROUP_ORDERS]


def status_batch(dtype):
    """[spd, zero_pivot_at(k = 599), spd_scaled, near_cancellation] at n = 600 and the statuses expected of them."""
    n = BATCH_ORDER
    base = family("spd", n, dtype)
    mats = [np.array(base), zero_pivot_at(base, BATCH_ZERO_STEP), np.array(family("spd_scaled", n, dtype)),
            near_cancellation(base, BATCH_CANCEL_STEP)]
    return mats, [STATUS_OK, STATUS_SINGULAR, STATUS_OK, STATUS_OK]


def side_by_side(n, dtype, copies=3):
    """One batch per order for the one-launch paths: all five families side by side, ``copies`` times over with other
    seeds, so that lane groups of different families share a wave at every lane count (8 members per wave at 8
    lanes).  Returns (members (5 * copies, n, n), family name of every member, seed of every member)."""
    mats, names, seeds = [], [], []
    for c in range(copies):
        for name in FAMILIES:
            s = seed_of(n) + 1000 * c
            if name == "tridiagonal":
                a = tridiagonal(n, dtype)
            else:
                a = {"spd": spd, "spd_scaled": spd_scaled, "spd_signed": spd_signed, "sparse_spd": sparse_spd}[name](
                    n, s, dtype)
            mats.append(a)
            names.append(name)
            seeds.append(s)
    return np.stack(mats), names, seeds
