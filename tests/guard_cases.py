"""Guarded buffers and the route tables of tests/test_gpu_memory_contract.py (tests/test_guard_cases.py proves the
checker on the CPU).  Pure numpy.

A dense call is handed views that sit INSIDE a larger buffer, an odd number of elements from its start, with margins on
both sides that hold a known bit pattern: a store one row, one padded column or one member outside the view changes a
margin, and a load from an input margin brings a NaN into a result that is compared bit for bit.

  * ``carve(shape, dtype, lead, fill_bits, margin)``: ``(whole, view)``.  ``whole`` is one flat array, every element
    of which holds ``fill_bits``; ``view`` has ``shape`` and starts ``front(margin) + lead`` elements in:
    ``front(margin)`` is the margin rounded up to a multiple of 64 elements, so with ``whole`` at an allocation's start
    (256 bytes or better) the view's address is ``lead`` elements past a 256-byte boundary.  ``lead = 1`` is "element
    aligned and nothing more" (address = one element mod 16 bytes, in fp32 and in fp64); a multiple of 64 is the
    aligned control.  ``margin = 0`` gives the plain reading: the view starts ``lead`` elements in.  Behind the view
    lie ``margin + lead`` elements more.
  * ``margin_for(n, cols)``: what a margin must hold for a route: two whole members plus two rows of the route's padded
    order.  No route pads an order beyond the next multiple of 512 (the widest outer block), so that is the padded
    order taken here for every route: a stray extra member or a row of padded stride cannot jump over such a margin.
  * ``intact(whole, span, fill_bits)``: the margins compared as integers, so a NaN whose payload changed and -0.0
    against +0.0 count as changes.
"""
from collections import namedtuple

import numpy as np

import overflow_cases as ovf
import wide_cases

F32, F64, I32 = np.float32, np.float64, np.int32
BITS = {4: np.uint32, 8: np.uint64}

# quiet NaNs with a payload one recognises in a failure message: what the input margins hold
NAN_IN = {F32: 0x7FC0DEAD, F64: 0x7FF80000DEADBEEF}
# what the margins (and, before the call, the views) of the outputs hold.  Floating point: a negative quiet NaN with a
# payload -- an arithmetic NaN has none, and every compared result is finite.  Status words are 0 ... 3 and a
# determinant's exponent is below 2^20 in magnitude for any matrix these formats hold.
SENTINEL = {F32: 0xFFC5A5A5, F64: 0xFFF85A5A5A5A5A5A, I32: 0x5A5A5A5A}
ALIGN = 64            # elements: 256 bytes in fp32 and int32, 512 in fp64
LEAD_ODD = 1          # address = one element mod 16 bytes
LEAD_ALIGNED = 64     # the control
# status words and determinant pairs: a member is one word and a one-launch workgroup holds at most 32 members
# (256 threads, 8 lanes each), so two "members" and two "rows" are far below this
WORD_MARGIN = 256


def _key(dtype):
    return np.dtype(dtype).type


def bits_of(x):
    """The array's elements as unsigned integers of their width (a view, not a copy)."""
    x = np.ascontiguousarray(x)
    return x.view(BITS[x.dtype.itemsize])


def front(margin):
    return -(-int(margin) // ALIGN) * ALIGN


def margin_for(n, cols=None):
    """Elements of margin for members of ``n`` rows and ``cols`` columns (``n`` where None; for ``solve`` the
    right-hand-side rows): two members and two rows of the padded order."""
    cols = n if cols is None else cols
    padded = -(-max(n, cols) // 512) * 512
    return 2 * n * cols + 2 * padded


def carve(shape, dtype, lead, fill_bits, margin=0):
    dtype = np.dtype(dtype)
    size = int(np.prod(shape, dtype=np.int64))
    start = front(margin) + int(lead)
    whole = np.empty(start + size + int(margin) + int(lead), dtype)
    bits_of(whole)[:] = fill_bits
    view = whole[start:start + size].reshape(shape)
    assert view.base is not None and np.shares_memory(view, whole)
    return whole, view


def span(whole, view):
    """(offset, elements) of the contiguous ``view`` inside ``whole``."""
    assert view.flags.c_contiguous and whole.ndim == 1 and view.dtype == whole.dtype
    off = (view.ctypes.data - whole.ctypes.data) // whole.itemsize
    assert 0 <= off and off + view.size <= whole.size
    return int(off), int(view.size)


Margins = namedtuple("Margins", "ok first changed")


def intact(whole, view_span, fill_bits):
    """``Margins(ok, first, changed)`` of a buffer ``carve`` made, after a call: ``changed`` margin elements differ from
    ``fill_bits`` as integers, the first of them at offset ``first`` relative to the view's start (negative: in front of
    the view; ``>= size``: behind it); ``first`` is None where the margins are intact."""
    off, size = view_span
    bits = bits_of(np.asarray(whole).reshape(-1))
    bad = bits != BITS[bits.dtype.itemsize](fill_bits)
    bad[off:off + size] = False
    where = np.flatnonzero(bad)
    if where.size == 0:
        return Margins(True, None, 0)
    return Margins(False, int(where[0]) - off, int(where.size))


def same_bits(got, want):
    """Equality of two arrays as bit patterns: dtype, shape and every bit."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and bool(np.array_equal(bits_of(got), bits_of(want)))


def first_difference(got, want):
    """For a failure message: how many elements differ as bits and the first of them, with both values."""
    got, want = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    if got.dtype != want.dtype or got.shape != want.shape:
        return {"dtype": (got.dtype, want.dtype), "shape": (got.shape, want.shape)}
    where = np.flatnonzero(bits_of(got) != bits_of(want))
    if where.size == 0:
        return None
    i = int(where[0])
    return {"differing": int(where.size), "first": i, "got": got[i], "want": want[i]}


# ---- the routes of tests/test_gpu_memory_contract.py -----------------------------------------------------------------
# One-launch kernels: 256 threads per workgroup (kResidentThreads), ``lanes`` of them per member, so a workgroup holds
# 256 / lanes members: one member more than that leaves the last wave and the last workgroup partly empty.
RESIDENT_THREADS = 256


def tail_batch(lanes):
    return RESIDENT_THREADS // lanes + 1


# reference: "steps" -- the step-by-step oracle of the dtype and pivoting (a zero multiplier skipped), "through" -- the
# same multiplying it through (the blocked fp32 route and the no-pivot blocked ones), "mirror64" -- matrix_inv_64_blocked
# at the resolved width.  batches: integers, or "tail" (tail_batch of the resolved lane count).
# expect: what the resolved_* queries must answer: an algorithm name of the package ("ALGO_..."), and for fp64 whether
# resolved_blocking_f64 is positive.
Route = namedtuple("Route", "name algo pivoting dtypes orders batches reference expect blocked64")

INV_ROUTES = [
    Route("resident", "workgroup", True, (F32, F64), (1, 8, 9, 33, 64), (1, "tail"), "steps", "ALGO_RESIDENT", False),
    Route("resident_nopivot", "workgroup", False, (F32, F64), (1, 8, 9, 33, 64), (1, "tail"), "steps", "ALGO_RESIDENT",
          False),
    Route("workgroup", "workgroup", True, (F32, F64), (65, 80, 81, 128), (1, 3), "steps", "ALGO_WORKGROUP", False),
    Route("wide", "wide", True, (F32,), tuple(wide_cases.EDGE_ORDERS), (1, 2), "steps", "ALGO_WIDE", False),
    Route("wide_nopivot", "wide", False, (F32,), tuple(wide_cases.EDGE_ORDERS), (1, 2), "steps", "ALGO_WIDE", False),
    Route("sweep32", "sweep", True, (F32,), (5, 257), (1,), "steps", "ALGO_SWEEP", False),
    Route("sweep64", "sweep", True, (F64,), (5, 255), (1,), "steps", "ALGO_SWEEP", False),
    Route("sweep_nopivot", "auto", False, (F32, F64), (100,), (1,), "steps", "ALGO_SWEEP", False),
    # 256: the order that needs no padding (np = 256); 16 pads 112 rows in front, 130 pads 126, 300 pads 84
    Route("blocked32", "blocked", True, (F32,), (16, 130, 256, 300), (1, 3), "through", "ALGO_BLOCKED", False),
    Route("blocked64", "auto", True, (F64,), (256, 300), (1,), "mirror64", None, True),
    Route("nopivot_blocked", "auto", False, (F32, F64), (520, 640), (1,), "through", "ALGO_BLOCKED", True),
]
# the smallest blocked fp32 shape that runs as two parts: a split needs 64 Mi elements and four members
# (mi32_plan.hip), and 1024 x 256^2 is that many at the order that needs no padding
SPLIT_ORDER, SPLIT_BATCH, SPLIT_DISTINCT = 256, 1024, 4

DET_ORDERS = tuple(ovf.DET_ORDERS)
# inv_det_any: (name, algo, pivoting, dtype, order, reference, block width query)
DetAny = namedtuple("DetAny", "name algo pivoting dtype n reference")
DET_ANY = [
    DetAny("blocked32", "auto", True, F32, 300, "through"),
    DetAny("blocked64", "auto", True, F64, 300, "mirror64"),
    DetAny("sweep32", "sweep", True, F32, 257, "steps"),
    DetAny("nopivot_blocked32", "auto", False, F32, 520, "through"),
    DetAny("nopivot_blocked64", "auto", False, F64, 520, "through"),
    DetAny("wide", "wide", True, F32, 129, "steps"),
]
SOLVE_ORDERS = (8, 33, 65, 100, 127)
SOLVE_K = (1, 3)
RESIDUAL_ORDERS = (65, 100)      # of residual_cases.FLOAT_ORDERS, off the 64-row tile edge: scalar and 16-byte loads
NULL_STATUS = [("one_launch", "workgroup", 33), ("sweep", "sweep", 100), ("blocked", "blocked", 130)]


def route_ids(routes):
    return [r.name for r in routes]
