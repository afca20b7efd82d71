"""Inputs and helpers of the determinant tests above order 128 (tests/test_det_large_mirror.py,
tests/test_gpu_det_large.py): the two pivot-reporting mirrors of tests/det_mirror_large.c -- (a) the step-by-step order,
row loop in parallel, (b) the fp64 blocked order -- built at test time like tests/det_mirror.c.  The recurrence that
turns pivots and swap flags into the (mantissa, exponent) pair stays det_cases.frexp_det."""
import ctypes
import os
import subprocess

import numpy as np

from det_cases import frexp_det

MIRROR_A_ORDERS = [129, 200, 257, 513]        # held to the oracle's step-by-step functions
MIRROR_B_SHAPES = [(n, bw) for bw in (64, 128) for n in (256, 300, 700)]  # held to gjo_matrix_inv_64_blocked


def _cpu_has(*flags):
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("flags"):
                    have = set(line.split(":", 1)[1].split())
                    return all(fl in have for fl in flags)
    except OSError:
        pass
    return False


def build_mirror_large(directory):
    """Compile tests/det_mirror_large.c into `directory` in the oracle's way: no contraction, every fused multiply-add
    spelled out; hardware FMA, AVX2 and OpenMP where the CPU and the compiler have them (the same bits either way: fma
    is correctly rounded in both, and a row's chain does not depend on which thread runs it)."""
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "det_mirror_large.c")
    lib = os.path.join(str(directory), "libdet_mirror_large.so")
    base = [os.environ.get("CC", "gcc"), "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-o", lib,
            src]
    fast = base + ["-O3", "-mavx2", "-mfma", "-fopenmp", "-lm"]
    if not (_cpu_has("avx2", "fma") and subprocess.call(fast, stderr=subprocess.DEVNULL) == 0):
        subprocess.check_call(base + ["-O2", "-Wno-unknown-pragmas", "-lm"])
    dll = ctypes.CDLL(lib)
    vp = ctypes.c_void_p
    for fn in (dll.detl_steps_f32, dll.detl_steps_f64):
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, ctypes.c_int, vp, vp, vp, ctypes.c_int]
    dll.detl_blocked_f64.restype = ctypes.c_int
    dll.detl_blocked_f64.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, vp]
    return dll


def mirror_steps(dll, a, pivoting=True):
    """Mirror (a): (inverse, status, pivot values, swap flags) of one float32 / float64 matrix."""
    a = np.ascontiguousarray(a)
    assert a.ndim == 2 and a.shape[0] == a.shape[1] and a.dtype in (np.float32, np.float64)
    n = a.shape[0]
    out = np.empty_like(a)
    piv = np.empty(n, a.dtype)
    swp = np.empty(n, np.int32)
    fn = dll.detl_steps_f32 if a.dtype == np.float32 else dll.detl_steps_f64
    st = fn(a.ctypes.data, n, out.ctypes.data, piv.ctypes.data, swp.ctypes.data, int(bool(pivoting)))
    return out, st, piv, swp != 0


def mirror_blocked64(dll, a, bw):
    """Mirror (b): the same four of one float64 matrix in the fp64 blocked order with blocks of bw columns."""
    a = np.ascontiguousarray(a, np.float64)
    n = a.shape[0]
    out = np.empty_like(a)
    piv = np.empty(n, np.float64)
    swp = np.empty(n, np.int32)
    st = dll.detl_blocked_f64(a.ctypes.data, n, int(bw), out.ctypes.data, piv.ctypes.data, swp.ctypes.data)
    return out, st, piv, swp != 0


def expected_pair(a, piv, swp, pivoting=True):
    m, e = frexp_det(a, piv, swp, pivoting)
    return np.float64(m), np.int32(e)


def signed_power_diagonal(n, seed):
    """(P D, mantissa, exponent): D a diagonal of signed powers of two, P a permutation matrix of its rows -- every
    pivot is +-2^k, exactly, whatever the elimination order, so the pair is known in closed form: mantissa
    +-0.5 with sign = parity(P) * prod sign(d), exponent = sum k + 1."""
    rng = np.random.default_rng(seed)
    k = rng.integers(-20, 21, n)
    sgn = rng.choice([-1.0, 1.0], n)
    perm = rng.permutation(n)
    a = np.zeros((n, n), np.float32)
    a[np.arange(n), perm] = (sgn * np.exp2(k)).astype(np.float32)  # row i holds d_i in column perm[i]
    seen = np.zeros(n, bool)
    cycles = 0
    for i in range(n):
        if not seen[i]:
            cycles += 1
            j = i
            while not seen[j]:
                seen[j] = True
                j = perm[j]
    sign = (-1.0) ** ((n - cycles) % 2) * np.prod(sgn)
    return a, np.float64(0.5 * sign), np.int32(int(k.sum()) + 1)
