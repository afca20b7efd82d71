"""Inputs and helpers of the solve tests (tests/test_solve_mirror.py, tests/test_solve_abi.py, tests/test_gpu_solve.py):
the step-by-step mirror of Gauss-Jordan on [A | B] (tests/solve_mirror.c), the right-hand sides, and the chunk rule of
include/mat_inv_32_c.h restated.  The matrix families are those of tests/det_cases.py."""
import ctypes
import os
import subprocess

import numpy as np


def build_solve_mirror(directory):
    """Compile tests/solve_mirror.c into `directory` with the host C compiler, in the oracle's way (no contraction:
    every fused multiply-add is spelled out), and load it."""
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "solve_mirror.c")
    lib = os.path.join(str(directory), "libsolve_mirror.so")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                           "-o", lib, src, "-lm"])
    dll = ctypes.CDLL(lib)
    for fn in (dll.solve_mirror_f32, dll.solve_mirror_f64):
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    return dll


def mirror_solve(dll, a, b, pivoting=True):
    """(X, status) of one float32 / float64 system: a is (n, n), b is (n, k) of a's dtype."""
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    assert a.ndim == 2 and a.shape[0] == a.shape[1] and a.dtype in (np.float32, np.float64)
    assert b.ndim == 2 and b.shape[0] == a.shape[0] and b.shape[1] >= 1 and b.dtype == a.dtype
    x = np.empty_like(b)
    fn = dll.solve_mirror_f32 if a.dtype == np.float32 else dll.solve_mirror_f64
    st = fn(a.ctypes.data, a.shape[0], b.ctypes.data, b.shape[1], x.ctypes.data, int(bool(pivoting)))
    return x, st


def mirror_solve_batch(dll, mats, rhs_batch, pivoting=True):
    """(X (B, n, k), statuses int32[B]) of a batch, member by member."""
    xs, sts = [], []
    for a, b in zip(mats, rhs_batch):
        x, st = mirror_solve(dll, a, b, pivoting)
        xs.append(x)
        sts.append(st)
    return np.stack(xs), np.array(sts, np.int32)


def rhs(n, k, seed, dtype=np.float32):
    """An (n, k) right-hand side drawn from U(-1, 1)."""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, k)).astype(dtype)


def cap(n):
    """The most right-hand-side columns one launch takes beside an order-n member."""
    return 64 - n if n <= 32 else 128 - n


def lanes_of(width):
    return 8 if width <= 8 else 16 if width <= 16 else 32 if width <= 32 else 64


def rows_of(n):
    return 40 if n <= 80 else 48 if n <= 96 else 56 if n <= 112 else 64


def expected_dispatch(n, nrhs):
    """(chunk_cols, launches, lanes, rows_per_thread) of mi32_resolve_solve for 1 <= n <= 127."""
    c = cap(n)
    width = n + min(nrhs, c)
    resident = width <= 64
    return c, -(-nrhs // c), lanes_of(width) if resident else 0, 0 if resident else rows_of(n)
