"""Inputs whose inverse overflows in known places while the status stays 0 (tests/test_overflow_cases.py proves them on
the CPU references, tests/test_gpu_overflow.py runs them on every inversion route).  Pure numpy, seeded.

The status looks at the input's entries and at the pivots only, so an inverse holding +-inf and NaN is a valid status-0
result, and the routes have to agree on it entry by entry.  A globally scaled matrix is no use for that (from n = 40 on
``gate * 2^-133`` comes out almost wholly NaN: a kernel that turned everything to NaN would nearly pass), so:

  * ``rows_down``: ``gate_matrix(n, 7000 + n)`` with every third row (1, 4, 7, ...) scaled by 2^-s, the product taken in
    float64 and then cast.  Partial pivoting takes the small rows last, so only the last third of the steps sees
    infinities and only the inverse's columns that belong to those rows overflow: the result is mostly finite, with
    infinities (sign included) and NaN in known positions.  The no-pivot twin takes ``nopivot_cases.spd``;
  * ``block_diag``: ``rows_down(n1)`` beside an ordinary ``gate_matrix(n2)`` (``spd(n2)``), exact zeros off the blocks,
    the overflowing block first or second.  Every multiplier between the blocks is an exact zero, which is where the
    two rules for a zero multiplier part: the reference skips the row update (the other block keeps its finite values),
    a kernel that multiplies through computes fma(-0, +-inf, x) = NaN.  On a dense ``rows_down`` both rules agree.

One integer step of s goes from "nothing overflows" to "a few columns survive", so the exponent of every
(pivoting, dtype, order) is a table entry here (``EXPONENT``), never computed by a test.

``ROUTES`` names, per route of the GPU file, the cases and WHICH REFERENCE applies:

  * ``skip``: the step-by-step oracle (the reference's rule): the sweep and the one-launch routes;
  * ``through``: the same oracle with ``zeros="through"``: the blocked fp32 route and the fp64 no-pivot blocked one;
  * ``mirror64``: ``matrix_inv_64_blocked`` at the resolved block width: the fp64 blocked route, whose composite order
    has an overflow boundary of its own.
"""
from collections import namedtuple

import numpy as np

from conftest import gate_matrix
from nopivot_cases import spd
from subnormal_cases import RAGGED_ORDERS, RESIDENT_ORDERS, WORKGROUP_ORDERS

F32, F64 = np.float32, np.float64
DTYPES = (F32, F64)
OK, SINGULAR = 0, 2
MIN_FINITE_SHARE = 0.25

# (pivoting, dtype) -> s of 2^-s; ``EXPONENT`` lists the orders that need another one
DEFAULT_EXPONENT = {(True, F32): 132, (True, F64): 1028, (False, F32): 126, (False, F64): 1022}
EXPONENT = {}
# (pivoting, order) -> seed of rows_down where 7000 + n does not meet the conditions: at order 8 the 8 + 8 block_diag
# with the overflowing block first keeps no infinity under the multiply-through rule with seed 7008
SEED = {(True, 8): 7012}

# kind: "rows_down" (n: the order), "block_diag" (n: (n1, n2), ``first``: the overflowing block comes first), "plain"
# (the ordinary gate_matrix / spd, for mixing into a batch); s: the exponent, 0 for "plain"
Case = namedtuple("Case", "kind dtype n pivoting first s")


def order(c):
    return sum(c.n) if c.kind == "block_diag" else c.n


def case(kind, dtype, n, pivoting=True, first=True, s=None):
    """A table entry; the exponent is ``EXPONENT``'s (the default of its (pivoting, dtype) where the order is not
    listed) unless the route names its own."""
    dtype = np.dtype(dtype).type
    if kind == "plain":
        return Case(kind, dtype, n, pivoting, True, 0)
    n1 = n[0] if kind == "block_diag" else n
    if s is None:
        s = EXPONENT.get((pivoting, dtype, n1), DEFAULT_EXPONENT[(pivoting, dtype)])
    return Case(kind, dtype, tuple(n) if kind == "block_diag" else n, pivoting, bool(first), s)


def base(n, pivoting, seed):
    """The ordinary matrix of order n, in float64."""
    return gate_matrix(n, seed).astype(F64) if pivoting else spd(n, seed, F64)


def rows_down(n, dtype, pivoting=True, s=None):
    """gate_matrix(n, 7000 + n) (spd for the no-pivot twin; ``SEED`` where listed) with the rows 1, 4, 7, ... scaled by
    2^-s."""
    if s is None:
        s = case("rows_down", dtype, n, pivoting).s
    a = base(n, pivoting, SEED.get((pivoting, n), 7000 + n))
    with np.errstate(under="ignore"):
        a[1::3] *= np.ldexp(1.0, -s)
        return a.astype(dtype)


def plain(n, dtype, pivoting=True):
    return base(n, pivoting, 7100 + n).astype(dtype)


def block_diag(n1, n2, dtype, first=True, pivoting=True, s=None):
    """rows_down(n1) beside plain(n2), exact zeros off the blocks; ``first``: the overflowing block comes first."""
    a = np.zeros((n1 + n2, n1 + n2), dtype)
    blocks = [rows_down(n1, dtype, pivoting, s), plain(n2, dtype, pivoting)]
    if not first:
        blocks.reverse()
    k = blocks[0].shape[0]
    a[:k, :k], a[k:, k:] = blocks
    return a


def matrix(c):
    if c.kind == "plain":
        a = plain(c.n, c.dtype, c.pivoting)
    elif c.kind == "rows_down":
        a = rows_down(c.n, c.dtype, c.pivoting, c.s)
    else:
        a = block_diag(c.n[0], c.n[1], c.dtype, c.first, c.pivoting, c.s)
    assert a.dtype == c.dtype and np.isfinite(a).all(), c
    return a


_WANT = {}


def reference(oracle, c, ref, bw=None):
    """(inverse (n, n), status) of case c on the reference ``ref``: ``"skip"`` / ``"through"``: the step-by-step oracle
    of c's dtype and pivoting with that rule for a zero multiplier; ``"mirror64"``: the fp64 blocked mirror at block
    width ``bw``.  Computed once per (case, reference, width), shared and read-only."""
    key = (c, ref, bw)
    if key not in _WANT:
        a, n = matrix(c), order(c)
        if ref == "mirror64":
            assert c.dtype == F64 and c.pivoting and bw
            x, info = oracle.matrix_inv_64_blocked(a, n, bw, return_info=True)
        elif not c.pivoting:
            x, info = oracle.matrix_inversion_no_pivots(a, n, return_info=True, zeros=ref)
        elif c.dtype == F32:
            x, info = oracle.matrix_inv_32_inplace(a, n, return_info=True, zeros=ref)
        else:
            x, info = oracle.matrix_inv_64(a, n, return_info=True, zeros=ref)
        x = x.reshape(n, n)
        x.setflags(write=False)
        _WANT[key] = (x, int(info["status"]))
    return _WANT[key]


def counts(x):
    """(share of finite entries, infinities, NaNs)."""
    x = np.asarray(x)
    return float(np.isfinite(x).mean()), int(np.isinf(x).sum()), int(np.isnan(x).sum())


def same_with_nonfinite(got, want):
    """subnormal_cases.same_with_nonfinite in the member's dtype: the same positions of non-finite entries, infinities
    with their sign and every NaN as one value, the finite entries byte for byte (-0.0 stored as +0.0)."""
    want = np.ascontiguousarray(want).reshape(-1)
    got = np.ascontiguousarray(got).reshape(-1)
    assert want.dtype in (F32, F64)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    nan, fin = np.isnan(want), np.isfinite(want)
    inf = ~nan & ~fin
    zero = want.dtype.type(0.0)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(np.isfinite(got), fin)
                and np.array_equal(got[inf], want[inf]) and (got[fin] + zero).tobytes() == (want[fin] + zero).tobytes())


def difference(got, want):
    """What a failed comparison is located by: how many entries differ under ``same_with_nonfinite``'s rule, the first of
    them (row-major) with both values, and the non-finite counts of both sides."""
    got, want = np.asarray(got), np.asarray(want).reshape(np.shape(got))
    with np.errstate(invalid="ignore"):
        bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    where = np.argwhere(bad)
    first = tuple(int(v) for v in where[0]) if len(where) else None
    return {"differing": len(where), "first": first, "got": None if first is None else float(got[first]).hex(),
            "want": None if first is None else float(want[first]).hex(), "got counts": counts(got),
            "want counts": counts(want)}


# ---- the routes of tests/test_gpu_overflow.py ------------------------------------------------------------------------
def _rd(dtype, orders, pivoting=True, s=None):
    return [case("rows_down", dtype, n, pivoting, s=s) for n in orders]


def _bd(dtype, pairs, pivoting=True, both=True):
    return [case("block_diag", dtype, p, pivoting, first) for p in pairs for first in ((True, False) if both else (True,))]


SMALL_PAIRS = [(8, 8), (40, 24)]
BLOCKED32_PAIRS = [(150, 150), (170, 130)]          # the second: the seam off the tile edge
BLOCKED32_BW128 = [(300, 8), (300, 32), (640, 8), (640, 32)]   # (order, panel width) at block_width = 128
BLOCKED32_BATCH_ORDER = 300
NOPIVOT_BLOCKED_PAIRS = [(456, 64), (600, 40)]      # orders 520 (padded) and 640 (not padded), seams off the tile edge
F64_BLOCKED_WIDTHS = (64, 128)                      # what resolved_blocking_f64 answers for block_width 64 and the default
# the overflowing block second: its infinities arise two and three outer blocks before the last one, so the pivot rows of
# the later rank-bw updates hold them as the B operand (in rows_down at s = 1027 they appear in the last update only)
BLOCKED64_BLOCK_DIAG = [case("block_diag", F64, (130, 170), first=False, s=1027),
                        case("block_diag", F64, (100, 200), first=False, s=1028)]
BLOCKED64_STATUS2 = case("rows_down", F64, 300, s=1028)   # the mirror flags it (status 2), the step oracle inverts it
DET_ORDERS = (8, 33, 64, 65, 128)
SOLVE_ORDERS = (8, 33, 65, 100)
SOLVE_K = 3

# route -> (reference, cases); "mirror64" cases are proved at every width of F64_BLOCKED_WIDTHS that the route runs
ROUTES = {
    "sweep32": ("skip", _rd(F32, (5, 64, 257)) + _bd(F32, SMALL_PAIRS)),
    "sweep64": ("skip", _rd(F64, (5, 64, 255)) + _bd(F64, SMALL_PAIRS)),
    "sweep_nopivot": ("skip", _rd(F32, (100,), False) + _rd(F64, (100,), False)),
    "blocked32": ("through", _rd(F32, (16, 130, 300))),
    "blocked32_bw128": ("through", _rd(F32, (300, 640))),
    "blocked32_block_diag": ("through", _bd(F32, [(8, 8)] + BLOCKED32_PAIRS)),
    "blocked32_nopivot": ("through", _rd(F32, (520, 640), False)),
    "blocked64": ("mirror64", _rd(F64, (300,), s=1027) + _rd(F64, (256,)) + BLOCKED64_BLOCK_DIAG),
    "nopivot64_blocked": ("through", _rd(F64, (520, 640), False) + _bd(F64, NOPIVOT_BLOCKED_PAIRS, False)),
    "host32": ("through", _rd(F32, (300,))),
    "host64": ("mirror64", _rd(F64, (300,), s=1027)),
    "host_nopivot": ("through", _rd(F64, (520,), False)),
    "residual": ("through", _rd(F32, (300,))),
    "det_large32": ("through", _rd(F32, (300,))),
    "det_large64": ("mirror64", _rd(F64, (300,), s=1027)),
    "det_large_nopivot": ("through", _rd(F32, (520,), False) + _rd(F64, (520,), False)),
}
ONE_LAUNCH_ORDERS = tuple(sorted(set(RESIDENT_ORDERS + WORKGROUP_ORDERS + RAGGED_ORDERS + DET_ORDERS + SOLVE_ORDERS)))


ONE_LAUNCH_SPLIT = {16: 8, 17: 11}   # order -> n1 where three quarters of the order do not meet the conditions


def one_launch_kinds(n):
    """The three members a one-launch batch of order n alternates: rows_down, block_diag (three quarters of the order in
    the overflowing block, which comes first; ``ONE_LAUNCH_SPLIT`` where listed) and an ordinary member.  Below order 8
    (order 3 of the mixed-order calls) no input meets the conditions: the member is an ordinary one."""
    if n < 8:
        return (("plain", n),) * 3
    n1 = ONE_LAUNCH_SPLIT.get(n, (3 * n) // 4)
    return ("rows_down", n), ("block_diag", (n1, n - n1)), ("plain", n)


def one_launch_cases(n, dtype, pivoting):
    return [case(kind, dtype, m, pivoting) for kind, m in one_launch_kinds(n)]


ROUTES["one_launch"] = ("skip", [c for dt in DTYPES for p in (True, False) for n in ONE_LAUNCH_ORDERS
                                 for c in one_launch_cases(n, dt, p) if c.kind != "plain"])


def widths_of(route, c):
    """The block widths at which a ``mirror64`` case is compared: both for the padded order 300, the default for 256."""
    if ROUTES[route][0] != "mirror64":
        return (None,)
    return F64_BLOCKED_WIDTHS if (route == "blocked64" and order(c) == 300) else (128,)


def table():
    """Every (route, reference, case, block width) of the table, once."""
    return [(route, ref, c, bw) for route, (ref, cs) in ROUTES.items() for c in cs for bw in widths_of(route, c)]


def mixed_batch(n, members, dtype, pivoting):
    """A uniform batch of ``members`` matrices of order n that alternates rows_down, block_diag and an ordinary member,
    so that one wave or workgroup class holds all three.  Returns (batch, cases)."""
    cs = [one_launch_cases(n, dtype, pivoting)[b % 3] for b in range(members)]
    return np.stack([matrix(c) for c in cs]), cs
