"""Inputs on gradual underflow (tests/test_subnormal_cases.py proves them on the CPU oracle and mirrors,
tests/test_gpu_subnormal.py runs them on every inversion path).  Pure numpy, seeded; every generator takes the dtype.

Once values are subnormal a scaling by a power of two is no relabelling of exponents: the oracle's result for
``gate * 2^-128`` is not ``2^128`` times its result for ``gate``, every step rounds on the subnormal grid.  Two
directions, for the pivoted paths and for the no-pivot ones:

  * ``down``: ``gate_matrix(n, seed) * 2^E`` with E = -128 (fp32) / -1024 (fp64), scaled in float64 and then cast: the
    INPUT is subnormal (every entry below 4 in magnitude before the scaling; the entries of about sqrt(n), and with
    them the pivots, are normal from n = 16 on), so are the multipliers' numerators and every intermediate of the
    columns still to be eliminated; the inverse is huge and ordinary;
  * ``up``: the same with E = +122 / +1018: the input is huge and finite, the INVERSE is subnormal, so every finished
    column and most of the later intermediates are;
  * ``det_down``: ``down`` with an exponent that follows the order, E = -126 (-1022) - ceil(log2(sqrt(n) + 1)): a
    pivot of gate_matrix is about sqrt(n), so from n = 16 on ``down``'s pivots are normal numbers again; here every
    pivot is subnormal at every order (the determinant's ``frexp`` is handed subnormal doubles in fp64) and the
    inverse, about 2^-E / sqrt(n), stays finite;
  * ``np_down``: ``nopivot_cases.spd(n, seed) * 2^E`` with E = -124 / -1018 (the diagonal stays normal, the rest not);
  * ``np_up``: ``(spd(n, seed) + 4 I) * 2^E`` with E = +121 / +1017.

The right-hand sides of the solves: ``solve down`` takes A as ``down`` and B = U(-1, 1) * 2^E with A's E (B wholly
subnormal, X ordinary); ``solve up`` takes A as ``up`` and B = U(-1, 1) unscaled (X subnormal).

``overflow_out``: ``gate_matrix(n, 5000 + n) * 2^-130`` at n = 3, 8, 16: every pivot is finite and the status is 0, but
the inverse overflows -- the status looks at pivots and input entries only.

``ROUTES`` names, for every route of the GPU file, the orders, dtypes and families it runs; the CPU file walks it.
"""
import numpy as np

from conftest import gate_matrix
from nopivot_cases import spd
from solve_cases import cap

F32, F64 = np.float32, np.float64
DTYPES = (F32, F64)
# family -> (fp32 exponent, fp64 exponent)
EXPONENTS = {"down": (-128, -1024), "up": (122, 1018), "np_down": (-124, -1018), "np_up": (121, 1017)}
PIVOTED = ("down", "up")
DET_PIVOTED = ("det_down", "up")
NOPIVOT = ("np_down", "np_up")
OVERFLOW_OUT_ORDERS = (3, 8, 16)
MIN_SHARE = 0.25          # of the input (down families) or of the expected output (up families)
MIN_SHARE_SOLVE_UP = 0.2  # of the X of ``solve up``


def share_subnormal(x):
    """The share of entries that are subnormal: non-zero and below the smallest normal number of x's dtype."""
    x = np.asarray(x)
    assert x.dtype in (F32, F64) and x.size
    m = np.abs(x)
    return float(((m > 0) & (m < np.finfo(x.dtype).tiny)).mean())


def exponent(family, dtype, n=None):
    """The power of two a family scales by; ``det_down``'s depends on the order."""
    f32 = np.dtype(dtype) == F32
    if family == "det_down":
        return (-126 if f32 else -1022) - int(np.ceil(np.log2(np.sqrt(n) + 1.0)))
    return EXPONENTS[family][0 if f32 else 1]


def seed_of(n):
    """One seed rule for every module that uses these families."""
    return 61_000 + n


def scaled(a, e, dtype):
    """a * 2^e, the product taken in float64 and then cast to ``dtype`` (round to nearest on the subnormal grid)."""
    with np.errstate(under="ignore"):
        return (np.asarray(a, F64) * np.ldexp(1.0, e)).astype(dtype)


def matrix(family, n, dtype, seed=None):
    """The member of ``EXPONENTS`` at order n; ``"gate"`` / ``"np_plain"``: the ordinary gate_matrix / spd, for mixing
    into a batch."""
    seed = seed_of(n) if seed is None else seed
    if family == "gate":
        return gate_matrix(n, seed).astype(dtype)
    if family == "np_plain":
        return spd(n, seed, dtype)
    if family in PIVOTED or family == "det_down":
        base = gate_matrix(n, seed)
    elif family == "np_down":
        base = spd(n, seed, F64)
    elif family == "np_up":
        base = spd(n, seed, F64) + 4.0 * np.eye(n)
    else:
        raise ValueError(family)
    a = scaled(base, exponent(family, dtype, n), dtype)
    assert np.isfinite(a).all(), (family, n, dtype)
    return a


def mixed_members(orders, dtype, families, seed0=0):
    """One member per entry of ``orders``, the families taken in turn (member b: families[b % len(families)]), every
    member with a seed of its own.  Returns (members, family of every member)."""
    mats, names = [], []
    for b, n in enumerate(int(n) for n in orders):
        names.append(families[b % len(families)])
        mats.append(matrix(names[-1], n, dtype, seed_of(n) + seed0 + 7 * b))
    return mats, names


def mixed_batch(n, members, dtype, families):
    """A uniform batch of ``members`` matrices of order n, the families alternating so that one wave holds all."""
    mats, names = mixed_members([n] * members, dtype, families)
    return np.stack(mats), names


def batch_families(pivoting):
    """The families a mixed batch alternates: the two subnormal ones and an ordinary member."""
    return ("down", "up", "gate") if pivoting else ("np_down", "np_up", "np_plain")


def solve_rhs(family, n, k, dtype, seed=None):
    """B of ``solve down`` (U(-1, 1) * 2^E, E that of ``down``) and of ``solve up`` (U(-1, 1) unscaled)."""
    assert family in PIVOTED
    seed = seed_of(n) + 500 if seed is None else seed
    b = np.random.default_rng([seed, n, k]).uniform(-1.0, 1.0, (n, k))
    return scaled(b, exponent("down", dtype), dtype) if family == "down" else b.astype(dtype)


def overflow_out(n):
    """fp32: gate_matrix(n, 5000 + n) * 2^-130.  Status 0 with an inverse that overflows."""
    return scaled(gate_matrix(n, 5000 + n), -130, F32)


def same_with_nonfinite(got, want):
    """Equality of float32 results that may hold non-finite entries: the same positions of non-finite entries,
    infinities with their sign and every NaN as one value (det_cases.same_doubles' rule), the finite entries bit for
    bit (-0.0 stored as +0.0, as conftest.canonical_bytes does)."""
    got = np.ascontiguousarray(got, F32).reshape(-1)
    want = np.ascontiguousarray(want, F32).reshape(-1)
    if got.shape != want.shape:
        return False
    nan, fin = np.isnan(want), np.isfinite(want)
    inf = ~nan & ~fin
    return (np.array_equal(np.isnan(got), nan) and np.array_equal(np.isfinite(got), fin)
            and np.array_equal(got[inf], want[inf])
            and (got[fin] + F32(0.0)).tobytes() == (want[fin] + F32(0.0)).tobytes())


# ---- the routes of tests/test_gpu_subnormal.py -----------------------------------------------------------------------
RESIDENT_ORDERS = (8, 9, 16, 17, 32, 33, 64)            # both sides of every lane class
WORKGROUP_ORDERS = (65, 80, 81, 96, 97, 112, 113, 128)  # both sides of every rows-per-thread class
RESIDENT_BATCH, WORKGROUP_BATCH = 16, 6
RAGGED_ORDERS = (3, 8, 9, 17, 33, 64, 65, 81, 97, 113, 128)
RAGGED_COPIES = 3
SOLVE_ORDERS = (8, 17, 33, 64, 65, 100, 127)
SOLVE_K = 3
SOLVE_TWO_CHUNK_ORDERS = (17, 100)                      # K = cap(n) + 1 there
# one solve_ragged call per K: every solve order at K = 3; at K = cap(100) + 1 (order 100 in two chunks, 127 in 29) the
# orders from 17 on -- at order 8 too little of the X of ``solve up`` is subnormal
SOLVE_RAGGED = {SOLVE_K: SOLVE_ORDERS, cap(100) + 1: SOLVE_ORDERS[1:]}
BLOCKED32_BW128 = [(300, 8), (300, 32), (640, 8), (640, 32)]   # (order, panel width) at block_width = 128
BLOCKED32_BATCH = (300, ("down", "up", "gate", "down"))

# route -> (dtypes, orders, families): what the GPU file runs, and what the CPU file proves the conditions for
ROUTES = {
    "sweep32": ((F32,), (5, 64, 257), PIVOTED),
    "blocked32": ((F32,), (300, 640), PIVOTED),
    "blocked32_bw128": ((F32,), (300, 640), PIVOTED),
    "blocked32_batch": ((F32,), (300,), PIVOTED),
    "nopivot32_sweep": ((F32,), (100,), NOPIVOT),
    "nopivot32_blocked": ((F32,), (512, 640), NOPIVOT),
    "sweep64": ((F64,), (5, 64, 255), PIVOTED),
    "blocked64": ((F64,), (256, 300), PIVOTED),
    "nopivot64_sweep": ((F64,), (100,), NOPIVOT),
    "nopivot64_blocked": ((F64,), (512, 640), NOPIVOT),
    "resident": (DTYPES, RESIDENT_ORDERS, PIVOTED),
    "resident_nopivot": (DTYPES, RESIDENT_ORDERS, NOPIVOT),
    "workgroup": (DTYPES, WORKGROUP_ORDERS, PIVOTED),
    "workgroup_nopivot": (DTYPES, WORKGROUP_ORDERS, NOPIVOT),
    "ragged": (DTYPES, RAGGED_ORDERS, PIVOTED),
    "det": (DTYPES, RESIDENT_ORDERS + WORKGROUP_ORDERS, DET_PIVOTED),
    "det_nopivot": (DTYPES, RESIDENT_ORDERS + WORKGROUP_ORDERS, NOPIVOT),
    "solve": (DTYPES, SOLVE_ORDERS, PIVOTED),
    "host32": ((F32,), (300,), PIVOTED),
    "host64": ((F64,), (300,), PIVOTED),
    "host_nopivot": ((F64,), (512,), NOPIVOT),
    "residual": ((F32,), (300,), PIVOTED),
}
F64_BLOCKED_WIDTHS = (64, 128)    # what resolved_blocking_f64 answers for block_width 64 and the default


def solve_shapes():
    """[(n, K)] of the uniform solve: K = 3 everywhere, and one column more than a launch takes at two orders."""
    return [(n, SOLVE_K) for n in SOLVE_ORDERS] + [(n, cap(n) + 1) for n in SOLVE_TWO_CHUNK_ORDERS]


def cases(route):
    """[(dtype, n, family)] of a route."""
    dtypes, orders, families = ROUTES[route]
    return [(dt, n, f) for dt in dtypes for n in orders for f in families]


def all_inversion_cases():
    """Every (dtype, n, family) some route inverts, once."""
    seen = []
    for route in ROUTES:
        for c in cases(route):
            if c not in seen:
                seen.append(c)
    return seen
