"""Inputs and helpers of the determinant tests (tests/test_det_mirror.py, tests/test_gpu_det.py): the step-by-step
mirror that reports pivot values (tests/det_mirror.c), the recurrence that turns them into the (mantissa, exponent)
pair of include/mat_inv_32_c.h, and the input families, which are those of tests/resident_cases.py."""
import ctypes
import math
import os
import subprocess

import numpy as np

from resident_cases import dist_matrix, dominant

KINDS = ("gate", "ref100", "rand", "hollow")
# the orders at which the mirror is held to the oracle: every lane count / rows-per-thread class and its edges
MIRROR_ORDERS = [1, 2, 3, 5, 8, 9, 16, 17, 31, 32, 33, 48, 63, 64, 65, 80, 81, 96, 97, 112, 113, 127, 128]
NOPIVOT_ORDERS = [1, 8, 9, 16, 17, 33, 64]
WORKGROUP_EDGES = [65, 80, 81, 96, 97, 112, 113, 128]
PERMUTATION_ORDERS = [2, 7, 20, 64, 65, 128]
STATUS_SINGULAR = 2


def build_mirror(directory):
    """Compile tests/det_mirror.c into `directory` with the host C compiler, in the oracle's way (no contraction:
    every fused multiply-add is spelled out), and load it."""
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "det_mirror.c")
    lib = os.path.join(str(directory), "libdet_mirror.so")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                           "-o", lib, src, "-lm"])
    dll = ctypes.CDLL(lib)
    for fn in (dll.det_mirror_f32, dll.det_mirror_f64):
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    return dll


def mirror(dll, a, pivoting=True):
    """(inverse, status, pivot values, swap flags) of one float32 / float64 matrix."""
    a = np.ascontiguousarray(a)
    assert a.ndim == 2 and a.shape[0] == a.shape[1] and a.dtype in (np.float32, np.float64)
    n = a.shape[0]
    out = np.empty_like(a)
    piv = np.empty(n, a.dtype)
    swp = np.empty(n, np.int32)
    fn = dll.det_mirror_f32 if a.dtype == np.float32 else dll.det_mirror_f64
    st = fn(a.ctypes.data, n, out.ctypes.data, piv.ctypes.data, swp.ctypes.data, int(bool(pivoting)))
    return out, st, piv, swp != 0


def frexp_det(a, pivots, swaps, pivoting=True):
    """The recurrence of include/mat_inv_32_c.h on the pivot values and swap flags of one member: (mantissa, exponent).
    A non-finite input entry: the accumulation never starts, (NaN, 0).  The step that meets a zero, NaN or infinite
    pivot ends it: (+0.0, 0) for an exactly zero pivot with pivoting on, (NaN, 0) otherwise."""
    if not np.isfinite(a).all():
        return math.nan, 0
    m, e = 1.0, 0
    for piv, swap in zip(pivots, swaps):
        piv = float(piv)  # exact for a float32
        if piv == 0.0 or not math.isfinite(piv):
            return (0.0 if pivoting and piv == 0.0 else math.nan), 0
        pm, pe = math.frexp(piv)
        if swap:
            m = -m
        m, k = math.frexp(m * pm)
        e += pe + k
    return m, e


def expected(dll, mats, pivoting=True):
    """(inverses, statuses, mantissas float64[B], exponents int32[B]) of a list or batch of members."""
    inv, st, mant, exp = [], [], [], []
    for a in mats:
        x, s, piv, swp = mirror(dll, a, pivoting)
        m, e = frexp_det(a, piv, swp, pivoting)
        inv.append(x)
        st.append(s)
        mant.append(m)
        exp.append(e)
    return inv, np.array(st, np.int32), np.array(mant, np.float64), np.array(exp, np.int32)


def same_doubles(got, want):
    """Equality of float64 arrays as bit patterns, with every NaN taken as one value (its payload is not defined)."""
    got = np.ascontiguousarray(got, np.float64)
    want = np.ascontiguousarray(want, np.float64)
    nan = np.isnan(want)
    return (got.shape == want.shape and np.array_equal(np.isnan(got), nan)
            and np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64)))


def family_members(n, dtype=np.float32):
    """One member per family at order n (hollow needs two rows), seeds as in the feasibility run: 7 + n."""
    return [dist_matrix(k, n, 7 + n).astype(dtype) for k in KINDS if not (k == "hollow" and n == 1)]


def dominant_member(n, dtype):
    return dominant(n, n, dtype)


def permutation_matrix(n, odd, dtype=np.float32):
    """A permutation matrix of the asked parity: a seeded shuffle, one more transposition where the parity is off."""
    perm = np.random.default_rng(90 + n).permutation(n)
    inversions = sum(int(perm[i] > perm[j]) for i in range(n) for j in range(i + 1, n))
    if (inversions % 2 == 1) != odd:
        perm[[0, 1]] = perm[[1, 0]]
    return np.eye(n, dtype=dtype)[perm]


def mixed_wave_orders():
    """Orders {3, 5, 8, 3, 7, ...} only: all in the 8-lane class, eight groups per wave, neighbours of different
    order -- a group must sit out the steps past its own order without accumulating in them."""
    return [3, 5, 8, 3, 7, 1, 8, 2, 6, 4, 8, 5, 3, 7, 2, 8, 1, 6, 5, 3, 8, 7, 4, 2] * 3
