"""Inputs and helpers of the relaxation tests (tests/test_relax_mirror.py, tests/test_relax_args.py,
tests/test_gpu_relax.py): the residual rule and the last fma of a sweep restated in C (tests/relax_mirror.c), the sweep
mirror built from it and tests/apply_mirror.c, and the test matrices.

A matrix here is ``(crow, col, val)`` in NumPy, int64 indices; a test narrows the indices where the call under test
takes int32.  Columns inside a row are in the order they were drawn unless a builder says otherwise: the stored order
is part of the definition."""
import ctypes
import os
import subprocess

import numpy as np

import stored_cases as sc
from apply_cases import mirror_apply


def build_relax_mirror(directory):
    """Compile tests/relax_mirror.c into `directory` the way ``apply_cases.build_apply_mirror`` compiles its source (no
    contraction: every fused multiply-add is spelled out), and load it."""
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "relax_mirror.c")
    lib = os.path.join(str(directory), "librelax_mirror.so")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                           "-o", lib, src, "-lm"])
    dll = ctypes.CDLL(lib)
    vp, ll = ctypes.c_void_p, ctypes.c_longlong
    for fn in (dll.residual_mirror_f32, dll.residual_mirror_f64):
        fn.restype, fn.argtypes = None, [ll] + [vp] * 7
    dll.axpy_mirror_f32.restype, dll.axpy_mirror_f32.argtypes = None, [ll, ctypes.c_float, vp, vp, vp]
    dll.axpy_mirror_f64.restype, dll.axpy_mirror_f64.argtypes = None, [ll, ctypes.c_double, vp, vp, vp]
    return dll


def _suffix(dtype):
    assert np.dtype(dtype) in (np.float32, np.float64)
    return "f32" if np.dtype(dtype) == np.float32 else "f64"


def mirror_residual(dll, csr, x, b, rows):
    """r of the rows `rows` (any order, repeats allowed), one entry per row."""
    crow, col = np.ascontiguousarray(csr[0], np.int64), np.ascontiguousarray(csr[1], np.int64)
    val = np.ascontiguousarray(csr[2])
    x, b = np.ascontiguousarray(x), np.ascontiguousarray(b)
    assert x.dtype == b.dtype == val.dtype and x.size == b.size == crow.size - 1
    assert col.size == 0 or (0 <= col.min() and col.max() < x.size)
    rows = np.ascontiguousarray(rows, np.int64)
    r = np.empty(rows.size, val.dtype)
    getattr(dll, "residual_mirror_" + _suffix(val.dtype))(rows.size, rows.ctypes.data, crow.ctypes.data, col.ctypes.data,
                                                          val.ctypes.data, x.ctypes.data, b.ctypes.data, r.ctypes.data)
    return r


def block_rows(first, orders):
    """The rows of the blocks one after the other: the packed layout of the residual."""
    return np.concatenate([np.arange(f, f + n, dtype=np.int64) for f, n in zip(first, orders)])


def mirror_axpy(dll, omega, z, x):
    """fma(omega, z, x) per element, one rounding."""
    z, x = np.ascontiguousarray(z), np.ascontiguousarray(x)
    assert z.dtype == x.dtype and z.shape == x.shape and z.ndim == 1
    out = np.empty_like(x)
    getattr(dll, "axpy_mirror_" + _suffix(x.dtype))(x.size, x.dtype.type(omega), z.ctypes.data, x.ctypes.data, out.ctypes.data)
    return out


def mirror_sweep(dll, adll, csr, first, wide, x, b, omega=1.0, sweeps=1):
    """x' of `sweeps` sweeps: this residual, then tests/apply_mirror.c (`adll`) on the widened members `wide`, then one
    fma.  Rows in no block keep x's value."""
    orders = [w.shape[0] for w in wide]
    rows = block_rows(first, orders)
    x = np.array(x, copy=True)
    for _ in range(sweeps):
        r = mirror_residual(dll, csr, x, b, rows)
        z, at = np.empty_like(r), 0
        for w in wide:
            n = w.shape[0]
            z[at:at + n] = mirror_apply(adll, w, r[at:at + n].copy().reshape(n, 1)).reshape(n)
            at += n
        new = x.copy()
        new[rows] = mirror_axpy(dll, omega, z, x[rows])
        x = new
    return x


def decode_store(data, orders, formats, dtype):
    """The members of a downloaded store (uint8 array), widened to `dtype`: what the sweep multiplies by."""
    off, _ = sc.offsets(orders, formats, dtype)
    out = []
    for n, f, o in zip(orders, formats, off):
        n, f = int(n), int(f)
        kind = {sc.NATIVE: dtype, sc.FLOAT32: np.float32, sc.FLOAT16: np.float16, sc.BFLOAT16: np.uint16}[f]
        raw = np.ascontiguousarray(data[o:o + n * n * sc.elem_bytes(f, dtype)]).view(kind)
        out.append(np.ascontiguousarray(sc.widen(raw, f, dtype).reshape(n, n)))
    return out


# ---- matrices ----
def csr_of_rows(cols, vals, dtype):
    """(crow, col, val) of per-row column and value arrays, in the order given."""
    crow = np.concatenate(([0], np.cumsum([len(c) for c in cols]))).astype(np.int64)
    col = np.concatenate([np.asarray(c, np.int64) for c in cols]) if crow[-1] else np.zeros(0, np.int64)
    val = np.concatenate([np.asarray(v, dtype) for v in vals]) if crow[-1] else np.zeros(0, dtype)
    return crow, col, val.astype(dtype)


def random_rows(n, lengths, seed, dtype, sort=False):
    """A matrix of n rows with `lengths[i]` entries in row i: distinct columns drawn from [0, n) in random order (sorted
    ascending with `sort`), values +-U(0.25, 1)."""
    rng = np.random.default_rng(seed)
    cols, vals = [], []
    for c in lengths:
        pick = rng.choice(n, int(c), replace=False)
        cols.append(np.sort(pick) if sort else pick)
        vals.append(rng.uniform(0.25, 1.0, int(c)) * rng.choice([-1.0, 1.0], int(c)))
    return csr_of_rows(cols, vals, dtype)


def first_of(orders):
    return np.concatenate(([0], np.cumsum(np.asarray(orders, np.int64))[:-1]))


JACOBI_ORDERS = list(range(1, 41)) + [64, 65, 100, 128]   # N = 1177


def jacobi_matrix(dtype, seed=5, off_block=4):
    """The convergence matrix: N = 1177, consecutive dense diagonal blocks of the orders JACOBI_ORDERS, `off_block`
    random entries per row outside the row's block, all off-diagonal values +-U(0.25, 1), and a_ii = 4 sum_{j != i}
    |a_ij| computed in float64 and rounded to `dtype`.  Columns ascending.  Returns (csr, orders, first)."""
    rng = np.random.default_rng(seed)
    orders = np.array(JACOBI_ORDERS)
    first = first_of(orders)
    n = int(orders.sum())
    cols, vals = [], []
    for f, m in zip(first, orders):
        for i in range(f, f + m):
            outside = np.concatenate((np.arange(0, f), np.arange(f + m, n)))
            c = np.concatenate((np.arange(f, f + m), rng.choice(outside, off_block, replace=False)))
            v = (rng.uniform(0.25, 1.0, c.size) * rng.choice([-1.0, 1.0], c.size)).astype(dtype).astype(np.float64)
            v[c == i] = 0.0
            v[c == i] = 4.0 * np.abs(v).sum()
            by = np.argsort(c)
            cols.append(c[by])
            vals.append(v[by])
    return csr_of_rows(cols, vals, dtype), orders, first


def dense_of(csr, dtype=np.float64):
    crow, col, val = csr
    n = crow.size - 1
    a = np.zeros((n, n), dtype)
    a[np.repeat(np.arange(n), np.diff(crow)), col] = val
    return a


def block_inverses(csr, orders, first, dtype):
    """The inverses of the diagonal blocks, computed in float64 and rounded to `dtype`."""
    a = dense_of(csr)
    return [np.ascontiguousarray(np.linalg.inv(a[f:f + n, f:f + n]).astype(dtype)) for f, n in zip(first, orders)]


def random_rows_fast(n, lengths, seed, dtype):
    """``random_rows`` for many rows, drawn in one piece: columns uniform in [0, n), so a row may hold a column twice
    (both entries are terms of the residual)."""
    rng = np.random.default_rng(seed)
    crow = np.concatenate(([0], np.cumsum(np.asarray(lengths, np.int64))))
    total = int(crow[-1])
    val = rng.uniform(0.25, 1.0, total) * rng.choice([-1.0, 1.0], total)
    return crow, rng.integers(0, n, total), val.astype(dtype)


def scaled_jacobi_matrix(dtype):
    """``jacobi_matrix`` with rows scaled by powers of two, so that the adaptive set-up chooses different storage formats
    for different blocks: every third block by 2^-24 as a whole (its inverse leaves float16's range), every third with
    alternate rows by 2^-12 (its condition number rules out the 16-bit formats), the rest as they are."""
    (crow, col, val), orders, first = jacobi_matrix(dtype)
    scale = np.ones(crow.size - 1)
    for k, (f, m) in enumerate(zip(first, orders)):
        if k % 3 == 1:
            scale[f:f + m] = 2.0 ** -24
        elif k % 3 == 2:
            scale[f:f + m:2] = 2.0 ** -12
    return (crow, col, (val * np.repeat(scale, np.diff(crow))).astype(dtype)), orders, first
