"""Python host side of the drop-in: the reference's call shapes over the C ABI.

* ``matrix_inv_32(vec, N)`` -- the library entry point
  (/root/reference/Matlab/mat_inv_32.h:4; MATLAB calls it as
  ``clib.matInv.matrix_inv_32(b, N)``, README.md:51): flat row-major fp32 in,
  flat row-major inverse out, EMPTY array for an invalid matrix (README.md:54).
* ``just_inv(K)`` -- the call shape of the reference's CPU script
  (/root/reference/matrix_inv_numpy.py:39-46): build a K x K U(0,100) matrix,
  time only the inversion with a monotonic clock, print ``TIME: <seconds>``.
* ``Inverter`` -- device-resident path for torch tensors (no host copies), used
  by bench.py and the multi-GPU driver.

PyTorch is plumbing only (device memory, streams); all arithmetic happens in
the HIP kernels of ``lib/libmat_inv_32.so``.
"""
from __future__ import annotations

import ctypes
import os
import time

import numpy as np

from . import _lib
from ._lib import (ALGO_AUTO, ALGO_BLOCKED, ALGO_NAMES, ALGO_RESIDENT, ALGO_SWEEP, ALGO_WIDE, ALGO_WORKGROUP, MI32_OK,
                   MI32_SINGULAR, Mi32Error)


def _algo_id(algo) -> int:
    if isinstance(algo, str):
        return ALGO_NAMES[algo.lower()]
    return int(algo)


def _call_flat(sym: str, matrix_vector, matrix_order: int, dtype, *extra):
    """``(rc, flat output)`` of the C entry point ``sym(vec, len, N, out, *extra)`` on a flat row-major ``dtype``
    copy of the input; None for a bad shape: ``N <= 0`` or ``int(len/N) != N`` (mat_inv_32.cpp:206-215)."""
    lib = _lib.load()
    n = int(matrix_order)
    v = np.ascontiguousarray(np.asarray(matrix_vector, dtype=dtype).reshape(-1))
    if n <= 0 or int(v.size // n) != n:
        return None
    out = np.empty(n * n, dtype=dtype)
    ptr = ctypes.POINTER(np.ctypeslib.as_ctypes_type(dtype))
    rc = getattr(lib, sym)(v.ctypes.data_as(ptr), v.size, n, out.ctypes.data_as(ptr), *extra)
    if rc == _lib.MI32_RUNTIME_ERROR:
        raise Mi32Error(lib.mi32_last_error().decode())
    return rc, out


def _invert_flat(sym: str, matrix_vector, matrix_order: int, dtype) -> np.ndarray:
    """The flat inverse, or an empty array where the reference returns an empty vector: a bad shape, or a singular
    input (README.md:54; ``MI32_SINGULAR_KEEP=1`` returns the shipped library's inf/NaN result instead)."""
    r = _call_flat(sym, matrix_vector, matrix_order, dtype)
    keep = os.environ.get("MI32_SINGULAR_KEEP", "0") not in ("", "0")
    if r is not None and (r[0] == MI32_OK or (r[0] == MI32_SINGULAR and keep)):
        return r[1]
    return np.empty(0, dtype=dtype)


def matrix_inv_32(matrix_vector, matrix_order: int) -> np.ndarray:
    """Drop-in for ``matrix_inv_32(std::vector<float>, int)``.

    Returns the flat row-major inverse (``float32``, ``N*N`` entries) or an empty
    array when the reference would return an empty vector: ``N <= 0``,
    ``int(len/N) != N`` (mat_inv_32.cpp:206-215), or a singular input (README.md:54;
    set ``MI32_SINGULAR_KEEP=1`` to get the shipped library's inf/NaN result instead).
    """
    return _invert_flat("mi32_matrix_inv_32", matrix_vector, matrix_order, np.float32)


def matrix_inv_64(matrix_vector, matrix_order: int) -> np.ndarray:
    """Drop-in for the reference's ``matrix_inversion_FP64(std::vector<double>, int)`` (headers.h:9): flat
    row-major float64 in, flat inverse out, empty array for a bad shape or a singular input."""
    return _invert_flat("mi32_matrix_inv_64", matrix_vector, matrix_order, np.float64)


def matrix_inversion_no_pivots(matrix_vector, matrix_order: int) -> np.ndarray:
    """Drop-in for the reference's ``matrix_inversion_no_pivots(std::vector<double>, int)`` (headers.h:11,
    matrix_inversion_no_pivots.cpp:10): Gauss-Jordan in double with the diagonal entry as every step's pivot --
    for diagonally dominant inputs.  Empty array for a bad shape, a non-finite input entry, or when a zero / non-finite
    diagonal entry is met.  From N = 512 on it runs on the blocked fp64 no-pivot path: the same result bit for bit
    (``np.array_equal``) as the step-by-step order, given finite intermediates; a zero multiplier is multiplied
    through there, so the sign of a zero entry can differ."""
    return _invert_flat("mi32_matrix_inversion_no_pivots", matrix_vector, matrix_order, np.float64)


def matrix_inv_32_batched(a: np.ndarray, ngpus: int = 1):
    """Host batch (B, N, N) -> (inverses (B, N, N), status int32[B]).  ``ngpus`` != 1: the batch is sharded over that
    many GPUs of this node (0 = all visible) inside the library, one host thread and context per GPU
    (``mi32_matrix_inv_32_batched_multi``): no launcher, no torch.distributed."""
    lib = _lib.load()
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 3 or a.shape[1] != a.shape[2] or a.shape[0] == 0 or a.shape[1] == 0:
        raise ValueError("expected a (B, N, N) array")
    b, n = a.shape[0], a.shape[1]
    out = np.empty_like(a)
    st = np.empty(b, dtype=np.int32)
    fp = ctypes.POINTER(ctypes.c_float)
    if ngpus != 1:
        rc = lib.mi32_matrix_inv_32_batched_multi(a.ctypes.data_as(fp), n, b, out.ctypes.data_as(fp),
                                                  st.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), int(ngpus))
        if rc == _lib.MI32_BAD_SHAPE:
            raise ValueError("more GPUs asked for than are visible")
    else:
        rc = lib.mi32_matrix_inv_32_batched(a.ctypes.data_as(fp), n, b, out.ctypes.data_as(fp),
                                            st.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    if rc == _lib.MI32_RUNTIME_ERROR:
        raise Mi32Error(lib.mi32_last_error().decode())
    return out, st


def _bench(sym: str, matrix_vector, matrix_order: int, dtype, *extra):
    """``(inverse, times)``; ``(empty, {})`` where the reference returns an empty Res."""
    times = (ctypes.c_double * 10)()
    r = _call_flat(sym, matrix_vector, matrix_order, dtype, times, *extra)
    if r is None or r[0] != MI32_OK:
        return np.empty(0, dtype=dtype), {}
    return r[1], dict(zip(_lib.TIMES10_SLOTS, (float(t) for t in times)))


def fp32_bench(matrix_vector, matrix_order: int):
    """The reference's ``Res FP32_bench(vector<float>, int)`` (FP32_bench.cpp:11): returns ``(inverse, times)``
    with ``times`` the ten durations of FP32_bench.cpp:256-443 in seconds, keyed by ``_lib.TIMES10_SLOTS``
    (queue, buffers, build, makeAug, pivot, row, column, compute, getInverted, total); ``(empty, {})`` where the
    reference returns an empty Res."""
    return _bench("mi32_bench_32", matrix_vector, matrix_order, np.float32)


def fp64_bench(matrix_vector, matrix_order: int, pivoting: bool = True):
    """``Res FP64_bench`` / ``Res no_pivots_bench`` of the reference (headers.h:14,16): ``(inverse float64, times)``.
    With ``pivoting=False`` from N = 512 on (the blocked no-pivot path), ``times["pivot"]`` is the diagonal blocks and
    ``times["column"]`` the block-column, strip and rank-bw updates; on the sweep kernels the pivot slot is 0."""
    return _bench("mi32_bench_64", matrix_vector, matrix_order, np.float64, 1 if pivoting else 0)


def matrix_multiply(matrice_a, matrice_b) -> float:
    """The reference's verification helper ``matrix_multiply`` (matrix_multiply.cpp:15): ``sqrt(N) - ||A B||_F`` with the
    product in double on the device; flat or square float64 operands of N*N entries each."""
    lib = _lib.load()
    a = np.ascontiguousarray(np.asarray(matrice_a, dtype=np.float64).reshape(-1))
    b = np.ascontiguousarray(np.asarray(matrice_b, dtype=np.float64).reshape(-1))
    if a.size != b.size:
        raise ValueError("operands of different size")
    err = ctypes.c_double()
    dp = ctypes.POINTER(ctypes.c_double)
    _lib.check(lib.mi32_matrix_multiply_64(a.ctypes.data_as(dp), b.ctypes.data_as(dp), a.size, ctypes.byref(err)),
               "mi32_matrix_multiply_64")
    return err.value


def last_timing():
    """(total_seconds, compute_seconds) of the last host-pointer call: the two numbers the
    reference prints (mat_inv_32.cpp:385-386)."""
    t, c = ctypes.c_double(), ctypes.c_double()
    _lib.load().mi32_last_timing(ctypes.byref(t), ctypes.byref(c))
    return t.value, c.value


def just_inv(K: int, seed=None, inv=None):
    """The reference CPU script's call shape (matrix_inv_numpy.py:39-46) on the GPU path:
    U(0,100) K x K matrix, time only the inversion, print ``TIME: <s>``.  Returns the
    elapsed seconds (the reference prints only).  ``inv`` lets the CPU-baseline harness
    time ``numpy.linalg.inv`` through the very same shape."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, 100, (K, K)).astype(np.float32)
    fn = inv if inv is not None else (lambda m: matrix_inv_32(m.reshape(-1), K))
    start = time.monotonic()
    res = fn(a)
    end = time.monotonic()
    print(f"TIME: {end - start}")
    return end - start, a, res


def slogdet_from_frexp(mant, exp):
    """``(sign, logabsdet)``, both float64, of determinants given as the pair ``det = mant * 2**exp`` that
    ``Inverter.inv_det`` and the ``det=True`` calls return: ``sign = torch.sign(mant)`` and ``logabsdet = log|mant| +
    exp * ln 2`` -- the layout of ``torch.linalg.slogdet``.  A zero mantissa gives ``(0, -inf)``, a NaN mantissa
    ``(NaN, NaN)``.  Pure torch: works on CPU tensors too."""
    import math

    import torch

    m = mant.to(torch.float64)
    sign = torch.where(torch.isnan(m), m, torch.sign(m))  # torch.sign alone turns a NaN into 0
    return sign, torch.log(torch.abs(m)) + exp.to(torch.float64) * math.log(2.0)


def det_from_frexp(mant, exp, dtype=None):
    """The determinants themselves, ``ldexp(mant, exp)``, as ``dtype`` (float64 by default).  Unlike the pair this can
    overflow to +-inf or underflow to 0: the determinant of 128 pivots of 2**100 is far outside any float format.  Use
    ``slogdet_from_frexp`` where the magnitude is not known to be moderate.  Pure torch: works on CPU tensors too."""
    import torch

    # in two halves: 2**exp alone may overflow or underflow where mant * 2**exp does not (the first product is exact)
    half = torch.div(exp, 2, rounding_mode="floor")
    d = mant.to(torch.float64) * torch.exp2(half.to(torch.float64)) * torch.exp2((exp - half).to(torch.float64))
    return d if dtype is None else d.to(dtype)


def vbatch_bin(orders):
    """``(perm, class_begin)`` of ``mi32_vbatch_bin`` (host only): the member indices sorted by order (stable) and the
    nine boundaries of the eight kernel classes in that list."""
    o, count = _order_array(orders)
    perm = np.empty(count, np.int32)
    begin = np.empty(9, np.int32)
    _lib.check(_lib.load().mi32_vbatch_bin(_int_ptr(o), count, _int_ptr(perm), _int_ptr(begin)), "mi32_vbatch_bin")
    return perm, begin


def _order_array(orders):
    """``(contiguous int32 array, its length)`` of ``orders``: what the host-only queries hand to the library."""
    o = np.ascontiguousarray(np.asarray(orders).reshape(-1), dtype=np.int32)
    return o, int(o.size)


def _int_ptr(array):
    return array.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def _ptr(t):
    """The address of a tensor as the library takes it; None stays None (a NULL argument)."""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _check_tensor(t, device, dtype, what, numel=None):
    """ValueError unless ``t`` is a contiguous 1-D tensor of ``dtype`` on ``device`` (of ``numel`` entries)."""
    if t.device != device:
        raise ValueError(f"{what} is on {t.device}, expected {device}")
    if t.dtype != dtype:
        raise ValueError(f"{what} is {t.dtype}, expected {dtype}")
    if t.dim() != 1 or not t.is_contiguous() or (numel is not None and t.numel() != numel):
        raise ValueError(f"{what}: expected a contiguous 1-D tensor" + (f" of {numel} entries" if numel else ""))


def _overlap(a, b):
    """Whether the storage spans of two contiguous tensors of one device meet."""
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def check_dense_args(device, a, out=None, status=None, *, b=None, want_inverse=True, max_order=None):
    """The argument handling of the dense calls, ``inv`` / ``inv_det`` / ``inv_det_any`` and, with ``b`` given,
    ``solve``: pure torch, no handle and no GPU (``device`` is the Inverter's; CPU tensors with
    ``torch.device("cpu")`` pass).  Everything a kernel would read or write is checked here, before any address is
    handed to the library; a refusal is a ValueError.

    * ``a``: float32 / float64 on ``device``, (N,N) or (B,N,N); a non-contiguous ``a`` is copied.
    * ``b`` (solve): a's dtype and device and a's batch dimension, then (N,) or (N,K).
    * ``out``: a's dtype on ``device``, contiguous, of ``B*N*N`` elements (solve: of b's shape); its storage span must
      not meet that of ``a`` anywhere.  In ``solve``, ``out`` may be ``b`` itself or cover exactly b's memory (in
      place); a partial overlap of the two is refused.
    * ``status``: a contiguous 1-D int32 tensor of ``B`` entries on ``device``.

    Returns ``(squeeze, a3, rhs, out3, status)``: the contiguous (B,N,N) input, the contiguous (B,N,K) right-hand side
    (None without ``b``), the output in that shape (allocated where ``out`` is None; None with
    ``want_inverse=False``) and the status tensor (allocated where None).  ``max_order``: the largest order
    ``inv_det`` takes."""
    import torch

    if a.dtype not in (torch.float32, torch.float64) or a.device != device:
        raise ValueError("expected a float32 or float64 tensor on the GPU" +
                         (f": a is on {a.device}, this Inverter on {device}" if a.device != device else ""))
    squeeze = a.dim() == 2
    a3 = a.unsqueeze(0) if squeeze else a
    if a3.dim() != 3 or a3.shape[1] != a3.shape[2] or a3.shape[0] == 0 or a3.shape[1] == 0:
        raise ValueError("expected (N,N) or (B,N,N)")
    bsz, n = a3.shape[0], a3.shape[1]
    if b is None:
        if max_order is not None and n > max_order:
            raise ValueError(f"inv_det takes orders up to {max_order}")
        b3 = None
    else:
        if n > 127:
            raise ValueError("solve takes orders up to 127")
        if b.dtype != a.dtype or b.device != a.device:
            raise ValueError(f"b is {b.dtype} on {b.device}, expected a's {a.dtype} on {a.device}")
        b3 = b.unsqueeze(-1) if b.dim() == a.dim() - 1 else b
        if squeeze:
            b3 = b3.unsqueeze(0)
        if b3.dim() != 3 or b3.shape[0] != bsz or b3.shape[1] != n or b3.shape[2] == 0:
            raise ValueError("b: expected a's batch dimension, then (N,) or (N,K)")
    if status is not None:
        _check_tensor(status, device, torch.int32, "status", bsz)
    if out is not None:
        if not want_inverse:
            raise ValueError("out given with want_inverse=False")
        if out.dtype != a.dtype or out.device != device:
            raise ValueError(f"out is {out.dtype} on {out.device}, expected {a.dtype} on {device}")
    a3 = a3.contiguous()
    if b is None:
        rhs = None
        if not want_inverse:
            out3 = None
        elif out is None:
            out3 = torch.empty_like(a3)
        else:
            if out.numel() != a3.numel():
                raise ValueError(f"out holds {out.numel()} elements, the result {a3.numel()}")
            if not out.is_contiguous() or _overlap(out, a3):
                raise ValueError("out must be contiguous and must not alias the input")
            out3 = out.view(bsz, n, n)
    elif out is None:
        rhs, out3 = b3.contiguous(), torch.empty(b3.shape, dtype=b.dtype, device=b.device)
    else:
        if out.shape != b.shape or not out.is_contiguous():
            raise ValueError("out: b itself or a contiguous tensor of b's shape, dtype and device")
        out3 = out.view(b3.shape)
        rhs = out3 if out is b else b3.contiguous()
        if _overlap(out3, a3):
            raise ValueError("out must not alias a")
        if rhs.data_ptr() != out3.data_ptr() and _overlap(out3, rhs):
            raise ValueError("out may be b itself (in place), not a part of b's memory")
    if status is None:
        status = torch.empty(bsz, dtype=torch.int32, device=device)
    return squeeze, a3, rhs, out3, status


# ---- the argument handling of the variable-size calls: pure torch like check_dense_args, no handle and no GPU.
# ``device`` is the Inverter's; of ``plan`` only ``batch``, ``flat_size``, ``total_rows``, ``orders``, ``device`` and
# whether ``_p`` is set are read, so any object with those attributes stands for a RaggedPlan.  Every refusal is a
# ValueError, raised before an address is formed. ----
def _check_float(dtype, what):
    import torch

    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what}: expected torch.float32 or torch.float64, not {dtype}")


def check_ragged_call(device, plan, dtype, status=None, *, max_order=128, want_status=True):
    """What every variable-size call checks first: ``plan`` is an open RaggedPlan of ``device`` whose largest order the
    call takes (``max_order``: 128 for ``inv`` and ``apply``, 127 for ``solve``); ``dtype``, the members' element type,
    is float32 or float64; ``status`` is None or a contiguous 1-D int32 tensor of ``plan.batch`` entries on ``device``.
    Returns the status tensor, allocated where None (None itself with ``want_status=False``: ``apply`` has none)."""
    import torch

    if not getattr(plan, "_p", None):
        raise ValueError("expected an open RaggedPlan")
    if plan.device != device:
        raise ValueError(f"the plan lives on {plan.device}, this Inverter on {device}")
    if int(plan.orders.max()) > max_order:
        raise ValueError(f"this call takes orders up to {max_order}: the plan holds an order-{int(plan.orders.max())} "
                         "member")
    _check_float(dtype, "dtype")
    if status is not None:
        _check_tensor(status, device, torch.int32, "status", plan.batch)
    elif want_status:
        status = torch.empty(plan.batch, dtype=torch.int32, device=device)
    return status


def check_pointer_args(device, plan, dtype, ptrs, lds, status=None, *, nrhs=1, **call):
    """The argument handling of ``inv_pointers`` / ``solve_pointers`` / ``apply_pointers``: ``check_ragged_call`` (which
    takes ``call``), then ``nrhs``, integral and at least 1; ``ptrs``, {name: tensor} of the member address arrays,
    contiguous 1-D int64 tensors of ``plan.batch`` entries on ``device``; ``lds``, the same for the leading dimensions,
    in int32 or None.  Returns the status tensor.  What the addresses point to cannot be checked, overlap included."""
    import torch

    status = check_ragged_call(device, plan, dtype, status, **call)
    if int(nrhs) != nrhs or nrhs < 1:
        raise ValueError("nrhs: at least one column")
    for what, t in ptrs.items():
        _check_tensor(t, device, torch.int64, what, plan.batch)
    for what, t in lds.items():
        if t is not None:
            _check_tensor(t, device, torch.int32, what, plan.batch)
    return status


def check_packed_matrices(device, plan, flat, what, status=None, **call):
    """The matrices of ``inv_ragged`` / ``solve_ragged`` / ``apply_ragged``: ``check_ragged_call`` (which takes
    ``call``) for flat's dtype, then ``flat`` itself, which holds the plan's members in the packed layout: a contiguous
    1-D tensor of ``plan.flat_size`` elements on ``device``.  Returns the status tensor."""
    status = check_ragged_call(device, plan, flat.dtype, status, **call)
    _check_tensor(flat, device, flat.dtype, what, plan.flat_size)
    return status


def check_diag_blocks(device, m, block_orders):
    """The block orders of ``inv_diag_blocks`` / ``solve_diag_blocks`` / ``apply_diag_blocks`` as an array: a non-empty
    1-D sequence that sums to the order of ``m``, a contiguous square float32 / float64 matrix on ``device``.
    ``m=None``: the blocks are stored packed, the orders may sum to anything."""
    orders = np.asarray(block_orders)
    if orders.ndim != 1 or orders.size == 0:
        raise ValueError("block_orders: a non-empty 1-D sequence of block orders")
    if m is not None:
        _check_float(m.dtype, "the matrix")
        if m.device != device:
            raise ValueError(f"the matrix is on {m.device}, expected {device}")
        if m.dim() != 2 or m.shape[0] != m.shape[1] or not m.is_contiguous():
            raise ValueError("expected a contiguous square matrix")
        if int(orders.sum()) != m.shape[0]:
            raise ValueError("block_orders must sum to the matrix order")
    return orders


def _check_out_alias(out, replaced, read=None):
    """The aliasing rule of the packed and diagonal-block calls, on contiguous tensors of one dtype and device:
    ``out`` may be the input it replaces -- the same address and the same extent, in place -- and otherwise meets it
    nowhere; it never meets ``read``, the matrices a ``solve`` or an ``apply`` reads."""
    if (out.data_ptr() != replaced.data_ptr() or out.numel() != replaced.numel()) and _overlap(out, replaced):
        raise ValueError("out may be the input it replaces (in place), not a part of its memory")
    if read is not None and _overlap(out, read):
        raise ValueError("out must not alias the matrices")


def check_inverse_out(src, out, shape, zero=False):
    """The output of ``inv_ragged`` / ``inv_diag_blocks`` for the input ``src`` (the packed members, or the matrix):
    ``out`` where given -- a contiguous tensor of ``shape`` and of src's dtype and device, ``src`` itself (in place) or
    memory that meets src's nowhere --, else a new tensor (``zero``: of zeros)."""
    import torch

    if out is None:
        return (torch.zeros if zero else torch.empty)(tuple(shape), dtype=src.dtype, device=src.device)
    if out.shape != tuple(shape) or out.dtype != src.dtype or out.device != src.device or not out.is_contiguous():
        raise ValueError(f"out: a contiguous tensor of shape {tuple(shape)} and of the input's dtype and device")
    _check_out_alias(out, src)
    return out


def check_packed_rhs(plan, mats, b, out, what):
    """The right-hand side of ``solve_ragged`` / ``solve_diag_blocks`` / ``apply_ragged`` / ``apply_diag_blocks``:
    ``b`` is ``(plan.total_rows,)`` or ``(plan.total_rows, K)``, K >= 1, of the dtype and device of ``mats`` (the checked
    matrices of the call), member i's rows starting at ``sum_{k<i} n_k``; ``out`` is None, ``b`` itself or a contiguous
    tensor of b's shape, dtype and device that meets neither b's memory nor that of ``mats``.  Returns
    ``(rhs, out, nrhs)``: ``rhs`` contiguous (a copy of a non-contiguous ``b``), ``out`` allocated where None, and 1
    column for a vector."""
    import torch

    if b.dtype != mats.dtype or b.device != mats.device:
        raise ValueError(f"{what} is {b.dtype} on {b.device}, expected {mats.dtype} on {mats.device}")
    if b.dim() not in (1, 2) or b.shape[0] != plan.total_rows or b.numel() == 0:
        raise ValueError(f"{what}: expected ({plan.total_rows},) or ({plan.total_rows}, K)")
    nrhs = 1 if b.dim() == 1 else int(b.shape[1])
    if out is None:
        return b.contiguous(), torch.empty(b.shape, dtype=b.dtype, device=b.device), nrhs
    if out.shape != b.shape or out.dtype != b.dtype or out.device != b.device or not out.is_contiguous():
        raise ValueError(f"out: {what} itself or a contiguous tensor of its shape, dtype and device")
    rhs = out if out is b else b.contiguous()
    _check_out_alias(out, rhs, mats)
    return rhs, out, nrhs


# ---- the sparse matrix of csr_diag_blocks / inv_csr_blocks: pure torch as above ----
def csr_parts(a):
    """``(crow, col, values)`` of the one argument form of the CSR calls: a 2-D square ``torch.sparse_csr`` tensor
    (through ``crow_indices()``, ``col_indices()`` and ``values()``), or the triple itself.  A batched CSR tensor, a
    tensor of another layout or a matrix that is not square is a ValueError."""
    import torch

    if isinstance(a, torch.Tensor):
        if a.layout != torch.sparse_csr:
            raise ValueError("expected a torch.sparse_csr tensor or a (crow, col, values) triple")
        if a.dim() != 2:
            raise ValueError("batched CSR tensors are not taken: expected a 2-D matrix")
        if a.shape[0] != a.shape[1]:
            raise ValueError(f"expected a square matrix, not {tuple(a.shape)}")
        return a.crow_indices(), a.col_indices(), a.values()
    if not isinstance(a, (tuple, list)) or len(a) != 3 or not all(isinstance(t, torch.Tensor) for t in a):
        raise ValueError("expected a torch.sparse_csr tensor or a (crow, col, values) triple")
    return tuple(a)


def check_csr(device, crow, col, values):
    """The CSR arrays of a square matrix: ``crow`` and ``col`` are contiguous 1-D tensors of ONE dtype, int32 or int64;
    ``values`` is a contiguous 1-D float32 / float64 tensor with col's element count; all three are on ``device`` and
    ``crow`` has at least 2 entries.  Returns ``N = crow.numel() - 1``.  What the arrays hold is not looked at (no
    synchronisation): that is ``validate_csr``."""
    import torch

    if crow.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"crow is {crow.dtype}, expected torch.int32 or torch.int64")
    if col.dtype != crow.dtype:
        raise ValueError(f"col is {col.dtype}, crow {crow.dtype}: expected one index dtype")
    _check_float(values.dtype, "values")
    _check_tensor(crow, device, crow.dtype, "crow")
    _check_tensor(col, device, col.dtype, "col")
    _check_tensor(values, device, values.dtype, "values")
    if values.numel() != col.numel():
        raise ValueError(f"values holds {values.numel()} entries, col {col.numel()}")
    if crow.numel() < 2:
        raise ValueError("crow: at least 2 entries (one row)")
    return crow.numel() - 1


def check_csr_first_rows(first_rows, orders, n):
    """The first row (and column) of every block as an int64 array, checked on the host: ``first_rows`` is a 1-D
    integer sequence with one entry per block, ``0 <= first`` and ``first + order <= n``.  Blocks may overlap or skip
    rows.  ``first_rows=None``: consecutive diagonal blocks, the orders must sum to ``n``."""
    orders = np.asarray(orders, dtype=np.int64)
    if first_rows is None:
        if int(orders.sum()) != n:
            raise ValueError(f"block_orders sum to {int(orders.sum())}, the matrix has {n} rows (or give first_rows)")
        return np.concatenate(([0], np.cumsum(orders)[:-1]))
    f = np.asarray(first_rows)
    if f.ndim != 1 or f.size != orders.size or not np.issubdtype(f.dtype, np.integer):
        raise ValueError(f"first_rows: a 1-D integer sequence of {orders.size} entries, one per block")
    f = f.astype(np.int64)
    if (f < 0).any() or (f + orders > n).any():
        b = int(np.nonzero((f < 0) | (f + orders > n))[0][0])
        raise ValueError(f"first_rows: block {b} (rows {int(f[b])} ... {int(f[b] + orders[b]) - 1}) leaves the matrix "
                         f"of {n} rows")
    return f


def check_csr_out(values, out, flat_size):
    """The packed output of ``csr_diag_blocks``: ``out`` where given -- a contiguous 1-D tensor of ``flat_size``
    elements of values' dtype and device that meets the memory of ``values`` nowhere --, else a new tensor."""
    import torch

    if out is None:
        return torch.empty(flat_size, dtype=values.dtype, device=values.device)
    _check_tensor(out, values.device, values.dtype, "out", flat_size)
    if _overlap(out, values):
        raise ValueError("out must not alias values")
    return out


def csr_pattern_parts(a):
    """``(crow, col)`` of the argument of the calls that read the sparsity pattern alone (``csr_block_starts`` /
    ``csr_find_blocks``): what ``csr_parts`` takes, and a ``(crow, col, None)`` triple."""
    import torch

    if isinstance(a, (tuple, list)) and len(a) == 3 and a[2] is None:
        if not all(isinstance(t, torch.Tensor) for t in a[:2]):
            raise ValueError("expected a torch.sparse_csr tensor or a (crow, col, values) triple")
        return a[0], a[1]
    return csr_parts(a)[:2]


def check_csr_pattern(device, crow, col):
    """``check_csr`` without the values: ``crow`` and ``col`` are contiguous 1-D tensors of ONE dtype, int32 or int64,
    on ``device``, and ``crow`` has at least 2 entries.  Returns ``N = crow.numel() - 1``.  No synchronisation."""
    import torch

    if crow.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"crow is {crow.dtype}, expected torch.int32 or torch.int64")
    if col.dtype != crow.dtype:
        raise ValueError(f"col is {col.dtype}, crow {crow.dtype}: expected one index dtype")
    _check_tensor(crow, device, crow.dtype, "crow")
    _check_tensor(col, device, col.dtype, "col")
    if crow.numel() < 2:
        raise ValueError("crow: at least 2 entries (one row)")
    return crow.numel() - 1


def check_find_blocks_args(max_order, agglomerate):
    """``(max_order, agglomerate)`` as the library takes them: an integer 1 ... 128 (a bool or a float is refused) and
    a bool."""
    if isinstance(max_order, bool) or not isinstance(max_order, (int, np.integer)):
        raise ValueError(f"max_order: expected an integer, not {type(max_order).__name__}")
    if not 1 <= int(max_order) <= _lib.CSR_FIND_MAX_ORDER:
        raise ValueError(f"max_order is {int(max_order)}, expected 1 ... {_lib.CSR_FIND_MAX_ORDER}")
    if not isinstance(agglomerate, (bool, np.bool_)):
        raise ValueError(f"agglomerate: expected a bool, not {type(agglomerate).__name__}")
    return int(max_order), bool(agglomerate)


def check_block_starts_out(crow, col, out, n):
    """The output of ``csr_block_starts``: ``out`` where given -- a contiguous 1-D uint8 tensor of ``n`` entries on
    crow's device that meets the memory of ``crow`` and ``col`` nowhere --, else a new tensor."""
    import torch

    if out is None:
        return torch.empty(n, dtype=torch.uint8, device=crow.device)
    if not isinstance(out, torch.Tensor):
        raise ValueError("out: expected a tensor")
    _check_tensor(out, crow.device, torch.uint8, "out", n)
    if _overlap(out, crow) or _overlap(out, col):
        raise ValueError("out must not alias crow or col")
    return out


def find_blocks_work_bytes(n):
    """``mi32_csr_find_blocks_work_bytes``: the temporary memory a call on ``n`` rows needs (host only)."""
    size = ctypes.c_size_t()
    _lib.check(_lib.load().mi32_csr_find_blocks_work_bytes(int(n), ctypes.byref(size)), "mi32_csr_find_blocks_work_bytes")
    return int(size.value)


def find_blocks_chunk_rows():
    """The rows of a chunk of ``csr_block_starts`` (host only): the orbit of row 0 is found chunk by chunk and chained,
    so this is where the seams are."""
    return int(_lib.load().mi32_csr_find_blocks_chunk_rows())


def validate_csr(crow, col, n):
    """What ``validate=True`` adds to ``check_csr``, each a ValueError: ``crow[0] == 0``, ``crow[-1] == nnz``, ``crow``
    non-decreasing, ``0 <= col < n``, no (row, column) pair twice.  Reads the arrays: synchronises."""
    import torch

    nnz = col.numel()
    if int(crow[0]) != 0:
        raise ValueError(f"crow[0] is {int(crow[0])}, expected 0")
    if int(crow[-1]) != nnz:
        raise ValueError(f"crow[-1] is {int(crow[-1])}, expected the {nnz} entries of col")
    counts = crow[1:] - crow[:-1]
    if bool((counts < 0).any()):
        raise ValueError("crow decreases")
    if nnz == 0:
        return
    if int(col.min()) < 0 or int(col.max()) >= n:
        raise ValueError(f"col: expected 0 <= col < {n}")
    rows = torch.repeat_interleave(torch.arange(n, device=col.device), counts.long())
    key = torch.sort(rows * n + col.long()).values
    if bool((key[1:] == key[:-1]).any()):
        at = int(key[1:][key[1:] == key[:-1]][0])
        raise ValueError(f"entry ({at // n}, {at % n}) is stored twice")


# ---- block inverses stored in a per-member format (store_inverses / apply_stored): pure torch and NumPy as above ----
class StorageFormat:
    """One row of ``STORAGE_FORMATS``: ``name``, ``nbytes`` per element (None: the working type's), the unit roundoff
    ``u``, the smallest normal and the largest finite magnitude (None for native, which always qualifies)."""

    def __init__(self, name, nbytes, u, smallest_normal, largest_finite):
        self.name, self.nbytes, self.u = name, nbytes, u
        self.smallest_normal, self.largest_finite = smallest_normal, largest_finite

    def __repr__(self):
        return f"StorageFormat({self.name})"


# the storage formats of include/mat_inv_32_stored.h by code
STORAGE_FORMATS = {
    0: StorageFormat("native", None, None, None, None),
    1: StorageFormat("float32", 4, 2.0 ** -24, 2.0 ** -126, (2.0 - 2.0 ** -23) * 2.0 ** 127),
    2: StorageFormat("float16", 2, 2.0 ** -11, 2.0 ** -14, 65504.0),
    3: StorageFormat("bfloat16", 2, 2.0 ** -8, 2.0 ** -126, (2.0 - 2.0 ** -7) * 2.0 ** 127),
}


def storage_candidates(dtype):
    """The format codes a member of ``dtype`` is tried in, narrowest first; native (0) is the fallback behind them."""
    import torch

    _check_float(dtype, "dtype")
    return (2, 3, 1) if dtype == torch.float64 else (2, 3)


def choose_storage(dtype, kappa, absmax, absmin, tol=0.1, status=None):
    """The storage format of every member, ``int32[batch]`` on the inputs' device: the first of float16, bfloat16,
    float32 (``dtype`` float64 only) for which ``kappa`` is finite, ``kappa * u_F <= tol``, ``absmax <=
    largest_finite_F`` and ``absmin >= smallest_normal_F``; native (0) otherwise, and for a member whose ``status`` is
    not 0.  ``kappa`` (``norm1(A) * norm1(X)`` as one float64 product), ``absmax`` and ``absmin`` (of X) are float64
    1-D tensors of one length and device, ``status`` an integer tensor beside them or None; ``tol`` is a positive
    number (0.1 is Ginkgo's).  Elementwise torch on float64, no kernel: CPU tensors pass."""
    import torch

    candidates = storage_candidates(dtype)
    for what, t in (("kappa", kappa), ("absmax", absmax), ("absmin", absmin)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.dim() != 1:
            raise ValueError(f"{what}: expected a 1-D float64 tensor")
        if t.shape != kappa.shape or t.device != kappa.device:
            raise ValueError(f"{what}: expected kappa's length and device")
    if not (isinstance(tol, (int, float)) and tol > 0 and tol < float("inf")):
        raise ValueError("tol: a positive finite number")
    open_ = torch.isfinite(kappa)
    if status is not None:
        if (not isinstance(status, torch.Tensor) or status.dtype.is_floating_point or status.shape != kappa.shape
                or status.device != kappa.device):
            raise ValueError("status: an integer tensor of kappa's length and device")
        open_ = open_ & (status == 0)
    out = torch.zeros(kappa.shape, dtype=torch.int32, device=kappa.device)
    for code in candidates:
        f = STORAGE_FORMATS[code]
        fits = open_ & (kappa * f.u <= tol) & (absmax <= f.largest_finite) & (absmin >= f.smallest_normal)
        out = torch.where(fits, torch.full_like(out, code), out)
        open_ = open_ & ~fits
    return out


def check_storage_formats(plan, dtype, formats):
    """The format codes of ``store_inverses`` as a host int32 array, checked on the host: ``formats`` is a 1-D integer
    sequence or an int32 tensor (a device tensor is downloaded: this synchronises) with one entry per member of
    ``plan``, every code one of ``STORAGE_FORMATS``, code 1 (float32) for float64 members only."""
    import torch

    _check_float(dtype, "dtype")
    if isinstance(formats, torch.Tensor):
        if formats.dtype != torch.int32:
            raise ValueError(f"formats is {formats.dtype}, expected torch.int32")
        f = formats.detach().cpu().numpy()
    else:
        f = np.asarray(formats)
    if f.ndim != 1 or f.size != plan.batch or not np.issubdtype(f.dtype, np.integer):
        raise ValueError(f"formats: a 1-D integer sequence of {plan.batch} entries, one per member")
    f = f.astype(np.int64)
    bad = ~np.isin(f, list(STORAGE_FORMATS))
    if dtype == torch.float32:
        bad |= f == 1
    if bad.any():
        b = int(np.nonzero(bad)[0][0])
        raise ValueError(f"formats: member {b} has code {int(f[b])}, which {dtype} members do not take")
    return f.astype(np.int32)


def stored_layout(orders, formats, native_bytes):
    """``(offsets, nbytes)`` of the store: member b starts at byte ``offsets[b]``, ``offsets[0] = 0`` and
    ``offsets[b + 1] = round_up_8(offsets[b] + n_b^2 * bytes(F_b))``; ``nbytes`` is what follows the last member in
    that way, the size of the buffer.  Host only: int64 arithmetic on the orders and the format codes."""
    size = np.array([native_bytes, 4, 2, 2], np.int64)[np.asarray(formats, np.int64)]
    span = (np.asarray(orders, np.int64) ** 2 * size + 7) // 8 * 8
    end = np.cumsum(span)
    return np.concatenate(([0], end[:-1])).astype(np.int64), int(end[-1])


def check_store_data(device, data, nbytes, x_flat=None):
    """A caller's buffer for the store: a contiguous 1-D uint8 tensor on ``device`` of at least ``nbytes`` bytes at an
    address that is a multiple of 8, which meets the memory of ``x_flat`` nowhere."""
    import torch

    _check_tensor(data, device, torch.uint8, "data")
    if data.numel() < nbytes or data.data_ptr() % 8:
        raise ValueError(f"data: at least {nbytes} bytes at an address that is a multiple of 8")
    if x_flat is not None and _overlap(data, x_flat):
        raise ValueError("data must not alias x_flat")


# ---- the vectors and blocks of csr_block_residual / relax_stored: pure torch and NumPy as above ----
def check_relax_vectors(values, n, x, b):
    """The iterate and the right-hand side of ``csr_block_residual`` / ``relax_stored``: ``x`` and ``b`` are contiguous
    1-D tensors of ``n`` entries, of the dtype and device of ``values`` (the checked values of the CSR matrix)."""
    import torch

    for what, t in (("x", x), ("b", b)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{what}: expected a tensor")
        _check_tensor(t, values.device, values.dtype, what, n)


def check_relax_out(values, out, numel, reads):
    """The output of ``csr_block_residual`` / ``relax_stored``: ``out`` where given -- a contiguous 1-D tensor of
    ``numel`` entries of values' dtype and device that meets none of ``reads``, {name: tensor or span} of everything
    the call reads --, else None (the caller allocates)."""
    import torch

    if out is None:
        return None
    if not isinstance(out, torch.Tensor):
        raise ValueError("out: expected a tensor")
    _check_tensor(out, values.device, values.dtype, "out", numel)
    for what, t in reads.items():
        if _overlap(out, t):
            raise ValueError(f"out must not alias {what}")
    return out


def check_blocks_disjoint(first, orders):
    """ValueError unless the blocks ``first[b] ... first[b] + orders[b] - 1`` (host arrays, ``check_csr_first_rows``)
    meet one another nowhere: a Jacobi sweep writes every row once."""
    first, orders = np.asarray(first, np.int64), np.asarray(orders, np.int64)
    by = np.argsort(first, kind="stable")
    ends = (first + orders)[by]
    clash = np.nonzero(ends[:-1] > first[by][1:])[0]
    if clash.size:
        a, b = int(by[clash[0]]), int(by[clash[0] + 1])
        raise ValueError(f"blocks {a} (rows {int(first[a])} ... {int(first[a] + orders[a]) - 1}) and {b} (from row "
                         f"{int(first[b])}) overlap: a relaxation sweep takes disjoint blocks")


def check_sweeps(sweeps, omega):
    """``(sweeps, omega)`` as the library takes them: an integer at least 1 (a bool or a float is refused) and a real
    number."""
    if isinstance(sweeps, bool) or not isinstance(sweeps, (int, np.integer)) or sweeps < 1:
        raise ValueError("sweeps: an integer, at least 1")
    if isinstance(omega, bool) or not isinstance(omega, (int, float, np.integer, np.floating)):
        raise ValueError(f"omega: expected a real number, not {type(omega).__name__}")
    return int(sweeps), float(omega)


class _StoreSpan:
    """The store's memory as ``check_packed_rhs`` looks at the matrices of a call: the members' dtype and device, and
    the span of the byte buffer."""

    def __init__(self, dtype, data):
        self.dtype, self.device, self._data = dtype, data.device, data

    def data_ptr(self):
        return self._data.data_ptr()

    def numel(self):
        return self._data.numel()

    def element_size(self):
        return 1


class StoredInverses:
    """What ``Inverter.store_inverses`` returns and ``Inverter.apply_stored`` takes: the members of ``plan`` (a
    RaggedPlan; it must stay open), of working type ``dtype``, each narrowed to its own storage format in one byte
    buffer.  ``formats`` (int32) and ``offsets`` (int64, bytes) are device tensors in the caller's member order,
    ``data`` the uint8 device buffer of ``nbytes`` bytes; ``native_nbytes`` is what the members take in ``dtype``,
    ``counts[code]`` the members per format.  Immutable by convention."""

    def __init__(self, plan, dtype, formats, offsets, data, nbytes, native_nbytes, counts):
        self.plan, self.dtype, self.formats, self.offsets, self.data = plan, dtype, formats, offsets, data
        self.nbytes, self.native_nbytes, self.counts = nbytes, native_nbytes, counts


class RaggedPlan:
    """A batch of members of mixed orders 1 ... 128 (``Inverter.plan_ragged``): the orders, binned once into the eight
    kernel classes and uploaded to the device.  Immutable; usable any number of times and from any ``Inverter`` on
    the same device.  ``close()`` frees its device memory and is safe while calls are still in flight."""

    def __init__(self, inverter, orders):
        torch = inverter._torch
        o = np.asarray(orders)
        if o.ndim != 1 or o.size == 0 or not (np.issubdtype(o.dtype, np.integer) or o.dtype == np.bool_):
            raise ValueError("orders: a non-empty 1-D sequence of integers")
        if o.min() < 1 or o.max() > 128:
            raise ValueError("orders must lie in 1 ... 128")
        self.orders = np.ascontiguousarray(o, dtype=np.int32)
        self.orders.setflags(write=False)
        self.batch = int(o.size)
        self.device = inverter.device
        self._lib = inverter._lib
        p = ctypes.c_void_p()
        _lib.check(self._lib.mi32_vbatch_create(inverter._h, self.orders.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                                self.batch, ctypes.byref(p)), "mi32_vbatch_create")
        self._p = p
        begin = (ctypes.c_int * 9)()
        _lib.check(self._lib.mi32_vbatch_info(self._p, None, begin), "mi32_vbatch_info")
        self.class_counts = [int(begin[k + 1] - begin[k]) for k in range(8)]
        sq = self.orders.astype(np.int64) ** 2
        self.flat_size = int(sq.sum())
        # element offset of every member in the packed layout: member b at sum_{i<b} n_i^2
        self._offsets = torch.from_numpy(np.concatenate(([0], np.cumsum(sq)[:-1]))).to(self.device)
        # the packed right-hand side of solve_ragged and apply_ragged: member b's rows start at sum_{i<b} n_i
        rows = self.orders.astype(np.int64)
        self.total_rows = int(rows.sum())
        self._row_offsets = torch.from_numpy(np.concatenate(([0], np.cumsum(rows)[:-1]))).to(self.device)
        self._torch = torch
        # (base address, dtype, nrhs or None, stream) -> int64 device tensor of member addresses.  The stream that
        # computed an entry is the only one that reads it, so dropping one is safe under the allocator's stream order.
        self._ptrs = {}

    def _pointers(self, t, nrhs, stream=None):
        """The cache behind ``packed_pointers`` (``nrhs=None``) and ``row_pointers``: at most 8 entries, cleared when
        full.  ``stream``: the current stream of the plan's device where the caller has looked it up already."""
        if stream is None:
            stream = self._torch.cuda.current_stream(self.device).cuda_stream
        key = (t.data_ptr(), t.dtype, nrhs, stream)
        ptrs = self._ptrs.get(key)
        if ptrs is None:
            if len(self._ptrs) >= 8:
                self._ptrs.clear()
            offsets, step = (self._offsets, 1) if nrhs is None else (self._row_offsets, nrhs)
            ptrs = self._ptrs[key] = offsets * (step * t.element_size()) + t.data_ptr()
        return ptrs

    def packed_pointers(self, flat):
        """int64 device tensor of the member addresses inside the packed tensor ``flat`` (cached per base, dtype and
        current stream)."""
        return self._pointers(flat, None)

    def row_pointers(self, t, nrhs):
        """int64 device tensor of the member addresses inside ``t``, a packed right-hand side of ``nrhs`` columns
        (member b's rows start at ``sum_{i<b} n_i``; cached per base, dtype, width and current stream: an iteration
        that uses the same buffers again computes nothing)."""
        return self._pointers(t, int(nrhs))

    def close(self):
        if getattr(self, "_p", None):
            self._lib.mi32_vbatch_destroy(self._p)
            self._p = None
            self._ptrs = {}

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class Inverter:
    """Device-resident inversion of torch CUDA(HIP) tensors through the C ABI handle."""

    def __init__(self, device=None, algo="auto", panel_width: int = 0, block_width: int = 0, pivoting: bool = True):
        import torch

        self._torch = torch
        if not torch.cuda.is_available():
            raise Mi32Error("no HIP device visible to torch; the product path has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else
                                   (device.index if isinstance(device, torch.device) else int(device)))
        self._lib = _lib.load()
        h = ctypes.c_void_p()
        _lib.check(self._lib.mi32_create(ctypes.byref(h), self.device.index), "mi32_create")
        self._h = h
        self.algo = _algo_id(algo)
        _lib.check(self._lib.mi32_set_algo(self._h, self.algo), "mi32_set_algo")
        if panel_width or block_width:
            _lib.check(self._lib.mi32_set_blocking(self._h, panel_width, block_width), "mi32_set_blocking")
        if not pivoting:  # the reference's no-pivot variant (matrix_inversion_no_pivots.cpp:10): blocked from 512 rows on
            _lib.check(self._lib.mi32_set_pivoting(self._h, 0), "mi32_set_pivoting")
        self._diag_plan = None  # (orders, plan, block offsets, leading dimensions) of the last inv_diag_blocks call

    def close(self):
        if getattr(self, "_diag_plan", None):
            self._diag_plan[1].close()
            self._diag_plan = None
        if getattr(self, "_h", None):
            self._lib.mi32_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _bind_stream(self):
        s = self._torch.cuda.current_stream(self.device)
        _lib.check(self._lib.mi32_set_stream(self._h, ctypes.c_void_p(s.cuda_stream)), "mi32_set_stream")
        return s.cuda_stream

    def _entry(self, stem, dtype):
        """The C entry point ``stem`` for float32 members, ``stem + "_f64"`` for float64 ones."""
        return getattr(self._lib, stem if dtype == self._torch.float32 else stem + "_f64")

    def resolved_algo(self, n: int, batch: int = 1) -> int:
        return self._lib.mi32_resolve_algo(self._h, int(n), int(batch))

    def resolved_blocking(self, n: int, batch: int = 1):
        """(sub-panel width, outer block width) the blocked path uses for this shape."""
        w, bw = ctypes.c_int(), ctypes.c_int()
        _lib.check(self._lib.mi32_resolve_blocking(self._h, int(n), int(batch), ctypes.byref(w), ctypes.byref(bw)),
                   "mi32_resolve_blocking")
        return w.value, bw.value

    def resolved_blocking_f64(self, n: int) -> int:
        """Outer block width of the fp64 blocked path for this order (with ``pivoting=False``: of the fp64 no-pivot
        path, 64 or 128); 0 where the unblocked sweep runs."""
        bw = ctypes.c_int()
        _lib.check(self._lib.mi32_resolve_blocking_f64(self._h, int(n), ctypes.byref(bw)), "mi32_resolve_blocking_f64")
        return bw.value

    def resolved_resident(self, n: int, elem_bytes: int = 4):
        """(lanes per matrix, largest order) of the register-resident path (``algo="resident"``): 8 / 16 / 32 / 64
        lanes for ``1 <= n <= 64``, 0 above, where that algorithm falls back to what ``auto`` resolves to."""
        lanes, top = ctypes.c_int(), ctypes.c_int()
        _lib.check(self._lib.mi32_resolve_resident(self._h, int(n), int(elem_bytes), ctypes.byref(lanes),
                                                   ctypes.byref(top)), "mi32_resolve_resident")
        return lanes.value, top.value

    def resolved_workgroup(self, n: int, elem_bytes: int = 4):
        """(threads per matrix, register rows per thread, largest order) of the workgroup-resident path
        (``algo="workgroup"``): 256 threads and 40 / 48 / 56 / 64 rows for ``65 <= n <= 128``; (0, 0, 128) outside,
        where that algorithm resolves to ``resident`` (``n <= 64``) or to what ``auto`` resolves to."""
        threads, rows, top = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _lib.check(self._lib.mi32_resolve_workgroup(self._h, int(n), int(elem_bytes), ctypes.byref(threads),
                                                    ctypes.byref(rows), ctypes.byref(top)), "mi32_resolve_workgroup")
        return threads.value, rows.value, top.value

    def resolved_wide(self, n: int, elem_bytes: int = 4):
        """(threads per matrix, register rows per thread, largest order) of the wide workgroup-resident path
        (``algo="wide"``, fp32 only): 768 threads and 40 / 48 rows for ``129 <= n <= 192``, 1024 threads and 56 / 64
        rows for ``193 <= n <= 256``; (0, 0, 256) outside and for ``elem_bytes=8``, where that algorithm resolves to
        ``resident`` (``n <= 64``), ``workgroup`` (``n <= 128``) or to what ``auto`` resolves to."""
        threads, rows, top = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _lib.check(self._lib.mi32_resolve_wide(self._h, int(n), int(elem_bytes), ctypes.byref(threads),
                                               ctypes.byref(rows), ctypes.byref(top)), "mi32_resolve_wide")
        return threads.value, rows.value, top.value

    def resolved_panel_widths(self, n: int, batch: int = 1):
        """Sub-panel width of every outer block (narrow while many rows are still candidates)."""
        nb = ctypes.c_int()
        buf = (ctypes.c_int * 128)()
        _lib.check(self._lib.mi32_resolve_panel_widths(self._h, int(n), int(batch), buf, 128, ctypes.byref(nb)),
                   "mi32_resolve_panel_widths")
        return [int(buf[i]) for i in range(min(nb.value, 128))]

    def resolved_route(self, n: int, batch: int = 1):
        """How a blocked fp32 call of this shape runs on this Inverter: (dict of the ``mi32_route_t`` fields -- shared
        panels, look-ahead, parts and where each part's strips run, first fused block --, workgroups per panel at the
        start of every outer block).  ValueError for an order the blocked path does not take."""
        return _lib.resolve_route(self._h, n, batch)

    def dominant_kernel(self, n: int, batch: int = 1) -> str:
        return self._lib.mi32_dominant_kernel(self.resolved_algo(n, batch)).decode()

    def reserve(self, n: int, batch: int = 1):
        _lib.check(self._lib.mi32_reserve(self._h, int(n), int(batch)), "mi32_reserve")

    def inv(self, a, out=None, status=None):
        """a: (N,N) or (B,N,N) float32 (or float64: the fp64 twin; sweep or blocked as resolved_blocking_f64
        reports) tensor on this device; a non-contiguous view is copied first, ``a`` is never modified.  ``out``
        (optional): a contiguous tensor of a's dtype on this device holding ``B*N*N`` elements, whose memory meets a's
        nowhere; it is returned, viewed as (B,N,N).  ``status`` (optional): a contiguous 1-D int32 tensor of ``B``
        entries on this device.  Anything else raises ValueError before the library is called
        (``check_dense_args``).  Element alignment is all ``a`` and ``out`` need, and nothing outside them, ``status``
        and the determinant pair is read or written.  Asynchronous on torch's current stream.  Returns (inverse,
        status int32[B] tensor)."""
        return self._dense("mi32_inv_device", a, out, status)

    def _dense(self, stem, a, out, status, want_inverse=True, max_order=None, det=False):
        """The one call behind ``inv``, ``inv_det`` and ``inv_det_any``: the arguments checked
        (``check_dense_args``), then the C entry point ``stem`` (float32) or ``stem + "_f64"`` on torch's current
        stream.  Returns ``(inverse, status)``; with ``det`` the entry point takes the two determinant arrays as well
        and they are returned behind, the inverse being None with ``want_inverse=False``."""
        torch = self._torch
        squeeze, a3, _, out, status = check_dense_args(self.device, a, out, status, want_inverse=want_inverse,
                                                       max_order=max_order)
        b, n = a3.shape[0], a3.shape[1]
        pair = (torch.empty(b, dtype=torch.float64, device=a3.device),
                torch.empty(b, dtype=torch.int32, device=a3.device)) if det else ()
        self._bind_stream()
        _lib.check(self._entry(stem, a.dtype)(self._h, _ptr(a3), n, b, _ptr(out), _ptr(status), *map(_ptr, pair)), stem)
        return ((None if out is None else out[0] if squeeze else out), status) + pair

    def inv_det(self, a, out=None, status=None, want_inverse=True):
        """The inverse and the determinant of every member from one launch.  a: (N,N) or (B,N,N) float32 / float64 on
        this device, N <= 128 (a larger N raises ValueError); ``out`` and ``status`` as for ``inv``.  Returns ``(inverse, status, det_mant, det_exp)``:
        ``det = det_mant * 2**det_exp`` with ``det_mant`` float64[B], ``|det_mant|`` in [0.5, 1), and ``det_exp``
        int32[B] (``slogdet_from_frexp`` / ``det_from_frexp`` turn the pair into log-determinant and sign, or the value).
        A singular member's pair is ``(0.0, 0)`` where an exactly zero pivot was met with pivoting on, ``(NaN, 0)``
        otherwise.  Inverse and status are those of ``inv`` bit for bit.  Always runs on the register-resident
        (N <= 64) or workgroup-resident kernels, whatever ``algo`` is.  ``want_inverse=False``: the determinant-only
        form, the inverse is not stored and None is returned in its place.  Asynchronous on torch's current stream."""
        return self._dense("mi32_inv_det_device", a, out, status, want_inverse, max_order=128, det=True)

    def inv_det_any(self, a, out=None, status=None, want_inverse=True):
        """``inv_det`` at any order ``inv`` takes.  Up to N = 128 it is ``inv_det``, same kernels and same bits.  Above,
        the call runs the route ``inv`` runs on this ``Inverter`` (algorithm, blocking, pivoting, look-ahead, batch
        split) and takes the determinant from that elimination's own pivots: inverse and status are ``inv``'s bit for
        bit, and the pair ``(det_mant, det_exp)`` follows the recurrence of ``inv_det`` over the pivots in step order.
        Returns ``(inverse, status, det_mant, det_exp)``.  ``want_inverse=False``: the elimination runs, the final
        un-permutation and store are skipped, and None is returned for the inverse.  With ``algo="wide"`` a float32
        batch of order 129 ... 256 takes the pair from the one launch of that path, as ``inv_det`` does below 129.
        Asynchronous on torch's current stream."""
        return self._dense("mi32_inv_det_any_device", a, out, status, want_inverse, det=True)

    def resolved_solve(self, n: int, nrhs: int, elem_bytes: int = 4):
        """(columns per launch, launches, lanes per member, register rows per thread) of ``solve`` for this shape: a
        call's ``nrhs`` columns are cut into chunks of at most ``64 - n`` (``n <= 32``) or ``128 - n`` columns, one
        launch each.  The last two describe the first chunk's kernel: 8 / 16 / 32 / 64 lanes and 0 rows where
        ``n`` plus the chunk fits 64 lanes (the register-resident kernel), 0 lanes and 40 / 48 / 56 / 64 rows where
        it takes the workgroup-resident one.  ``n > 127`` or ``nrhs < 1`` raises ValueError."""
        cols, launches, lanes, rows = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _lib.check(self._lib.mi32_resolve_solve(self._h, int(n), int(nrhs), int(elem_bytes), ctypes.byref(cols),
                                                ctypes.byref(launches), ctypes.byref(lanes), ctypes.byref(rows)),
                   "mi32_resolve_solve")
        return cols.value, launches.value, lanes.value, rows.value

    def solve(self, a, b, out=None, status=None):
        """X with A X = B for every member, without forming the inverse: Gauss-Jordan on [A | B] in the one-launch
        batch kernels.  a: (N,N) or (B,N,N) float32 / float64 on this device, N <= 127 (a larger N raises ValueError).
        b: a's dtype and device and a's batch dimension, then (N,) -- one vector per member, the result keeps that
        shape -- or (N,K).  ``out`` may be ``b`` itself (in place) or a contiguous tensor of b's shape, dtype and device;
        its memory must meet a's nowhere, and b's either wholly (in place) or not at all.  ``status`` (optional): a
        contiguous 1-D int32 tensor of ``B`` entries on this device.  Anything else raises ValueError before the library
        is called (``check_dense_args``).  ``a`` is never modified, ``b`` only in place; element alignment is all the
        three need.  Returns ``(x, status int32[B])``; x of a member whose status is not 0 is unspecified.  With
        ``b`` the identity, x is ``inv``'s result bit for bit.  More than ``resolved_solve(N, K)[0]`` columns take one
        launch per chunk, and every launch repeats the elimination of A.  Always runs on the register-resident or
        workgroup-resident kernels, whatever ``algo`` is.  Asynchronous on torch's current stream."""
        _, a3, rhs, out3, status = check_dense_args(self.device, a, out, status, b=b)
        bsz, n = a3.shape[0], a3.shape[1]
        self._bind_stream()
        _lib.check(self._entry("mi32_solve_device", a.dtype)(self._h, _ptr(a3), n, bsz, _ptr(rhs), rhs.shape[2],
                                                             _ptr(out3), _ptr(status)), "mi32_solve_device")
        return out3.view(b.shape), status

    # ---- variable-size batches: mixed orders 1 ... 128, each member at its own pointer and leading dimension ----
    def plan_ragged(self, orders) -> RaggedPlan:
        """Bin a batch of members of the given orders (a sequence or an int array, each 1 ... 128) once."""
        return RaggedPlan(self, orders)

    def inv_pointers(self, plan, a_ptrs, out_ptrs, dtype, lda=None, ldout=None, status=None, *, det=False):
        """The low-level form: ``a_ptrs`` / ``out_ptrs`` are int64 device tensors of ``plan.batch`` member addresses
        (row-major members of ``dtype`` float32 / float64), ``lda`` / ``ldout`` int32 device tensors of leading
        dimensions in elements (None: the member's order).  A member may be inverted in place (same address, same
        leading dimension); members that overlap otherwise are undefined.  Asynchronous on torch's current stream.
        Returns the status tensor (int32[batch], the caller's member order).  ``det=True``: the determinants come
        from the same launches and ``(status, (det_mant, det_exp))`` is returned (float64[batch] and int32[batch] in
        the caller's member order, the pair of ``inv_det``); ``out_ptrs=None`` is then the determinant-only form."""
        if out_ptrs is None and not det:
            raise ValueError("out_ptrs=None needs det=True (the determinant-only form)")
        ptrs = {"a_ptrs": a_ptrs} if out_ptrs is None else {"a_ptrs": a_ptrs, "out_ptrs": out_ptrs}
        status = check_pointer_args(self.device, plan, dtype, ptrs, {"lda": lda, "ldout": ldout}, status)
        self._bind_stream()
        return self._inv_vbatched(plan, dtype, a_ptrs, lda, out_ptrs, ldout, status, det)

    def _inv_vbatched(self, plan, dtype, a_ptrs, lda, out_ptrs, ldout, status, det):
        """The library call of the variable-size inversions, on the stream bound; ``status``, or with ``det``
        ``(status, (det_mant, det_exp))``."""
        torch = self._torch
        pair = (torch.empty(plan.batch, dtype=torch.float64, device=self.device),
                torch.empty(plan.batch, dtype=torch.int32, device=self.device)) if det else ()
        stem = "mi32_inv_det_device_vbatched" if det else "mi32_inv_device_vbatched"
        _lib.check(self._entry(stem, dtype)(self._h, plan._p, _ptr(a_ptrs), _ptr(lda), _ptr(out_ptrs), _ptr(ldout),
                                            _ptr(status), *map(_ptr, pair)), stem)
        return (status, pair) if det else status

    def inv_ragged(self, plan, a_flat, out=None, status=None, *, det=False):
        """The packed layout: ``a_flat`` is a 1-D float32 / float64 device tensor in which member b holds its
        ``n_b * n_b`` row-major elements at offset ``sum_{i<b} n_i^2``.  One call, at most eight launches.  ``out``
        may be ``a_flat`` itself (in place) and otherwise meets its memory nowhere.  Returns ``(out_flat, status)``;
        with ``det=True`` ``(out_flat, status, (det_mant, det_exp))``, the pair of ``inv_det`` in the caller's member
        order."""
        status = check_packed_matrices(self.device, plan, a_flat, "a_flat", status)
        out = check_inverse_out(a_flat, out, a_flat.shape)
        stream = self._bind_stream()
        r = self._inv_vbatched(plan, a_flat.dtype, plan._pointers(a_flat, None, stream), None,
                               plan._pointers(out, None, stream), None, status, det)
        return (out, r[0], r[1]) if det else (out, r)

    def resolved_solve_ragged(self, orders, nrhs: int):
        """The launches of one ``solve_pointers`` / ``solve_ragged`` / ``solve_diag_blocks`` call on members of these
        orders (each 1 ... 127) with ``nrhs`` columns, host only: a list of ``(first, count, col0, cols, lanes, rows)``
        -- a range of the member list sorted by order, the columns of B, and the kernel instance as ``resolved_solve``
        names it (lanes per member, or 0 and the workgroup-resident kernel's rows per thread).  Every member runs as
        ``solve`` would run a uniform batch of its order; members whose chunks agree share their launches, so
        ``nrhs = 1`` takes at most eight.  An order outside 1 ... 127 or ``nrhs < 1`` raises ValueError."""
        o, size = _order_array(orders)
        count = ctypes.c_int()
        _lib.check(self._lib.mi32_vbatch_solve_launches(_int_ptr(o), size, int(nrhs), None, 0, ctypes.byref(count)),
                   "mi32_vbatch_solve_launches")
        out = np.empty((count.value, 6), np.int32)
        _lib.check(self._lib.mi32_vbatch_solve_launches(_int_ptr(o), size, int(nrhs), _int_ptr(out), count.value,
                                                        ctypes.byref(count)), "mi32_vbatch_solve_launches")
        return [tuple(int(v) for v in row) for row in out]

    def solve_pointers(self, plan, a_ptrs, b_ptrs, x_ptrs, dtype, nrhs, lda=None, ldb=None, ldx=None, status=None):
        """A X = B for every member of the plan in one call, the low-level form: ``a_ptrs`` / ``b_ptrs`` / ``x_ptrs``
        are int64 device tensors of ``plan.batch`` member addresses (row-major members of ``dtype`` float32 / float64:
        A is n x n, B and X are n x ``nrhs``), ``lda`` / ``ldb`` / ``ldx`` int32 device tensors of leading dimensions
        in elements (None: the member's order for ``lda``, ``nrhs`` for the other two).  A member may be solved in
        place (the same address and leading dimension for B and X); X over A, or members that overlap otherwise, are
        undefined.  ``nrhs < 1`` or a plan that holds an order-128 member raises ValueError.  Every member is
        ``solve``'s result for its order bit for bit; ``resolved_solve_ragged`` lists the launches.  Asynchronous on
        torch's current stream.  Returns the status tensor (int32[batch], the caller's member order)."""
        status = check_pointer_args(self.device, plan, dtype, {"a_ptrs": a_ptrs, "b_ptrs": b_ptrs, "x_ptrs": x_ptrs},
                                    {"lda": lda, "ldb": ldb, "ldx": ldx}, status, nrhs=nrhs, max_order=127)
        self._bind_stream()
        return self._solve_vbatched(plan, dtype, nrhs, a_ptrs, lda, b_ptrs, ldb, x_ptrs, ldx, status)

    def _solve_vbatched(self, plan, dtype, nrhs, a_ptrs, lda, b_ptrs, ldb, x_ptrs, ldx, status):
        """The library call of the variable-size solves, on the stream bound; returns ``status``."""
        _lib.check(self._entry("mi32_solve_device_vbatched", dtype)(
            self._h, plan._p, _ptr(a_ptrs), _ptr(lda), _ptr(b_ptrs), _ptr(ldb), int(nrhs), _ptr(x_ptrs), _ptr(ldx),
            _ptr(status)), "mi32_solve_device_vbatched")
        return status

    def solve_ragged(self, plan, a_flat, b, out=None, status=None):
        """A X = B for members of mixed orders 1 ... 127 in one call.  ``a_flat`` is the packed layout of
        ``inv_ragged``; ``b`` is a contiguous ``(plan.total_rows,)`` or ``(plan.total_rows, K)`` tensor of a_flat's
        dtype and device in which member i's rows start at ``sum_{k<i} n_k`` (a vector keeps its shape).  ``out`` may
        be ``b`` itself (in place) or a contiguous tensor of its shape that meets b's memory nowhere; it never meets
        that of ``a_flat``.  Returns
        ``(x, status)``; x of a member whose status is not 0 is unspecified.  A plan that holds an order-128 member
        raises ValueError."""
        status = check_packed_matrices(self.device, plan, a_flat, "a_flat", status, max_order=127)
        rhs, out, nrhs = check_packed_rhs(plan, a_flat, b, out, "b")
        stream = self._bind_stream()
        return out, self._solve_vbatched(plan, a_flat.dtype, nrhs, plan._pointers(a_flat, None, stream), None,
                                         plan._pointers(rhs, nrhs, stream), None, plan._pointers(out, nrhs, stream),
                                         None, status)

    def solve_diag_blocks(self, m, block_orders, r, out=None):
        """``z = blockdiag(m)^-1 r``, the application of a block-Jacobi preconditioner, in one call: the consecutive
        diagonal blocks of the square device matrix ``m`` have the orders ``block_orders`` (each 1 ... 127, summing to
        ``m.shape[0]``), ``r`` is ``(N,)`` or ``(N, K)`` of m's dtype and device.  Only the block entries of ``m`` are
        read and no inverse is formed.  ``out`` as in ``solve_ragged``, with ``m`` for ``a_flat``.  Returns ``(z, status)``
        with one status word per block.  The plan of the last block structure is kept (shared with ``inv_diag_blocks``)."""
        plan, elem_off, lds = self._diag_blocks_plan(m, block_orders)
        status = check_ragged_call(self.device, plan, m.dtype, max_order=127)
        rhs, out, nrhs = check_packed_rhs(plan, m, r, out, "r")
        stream = self._bind_stream()
        return out, self._solve_vbatched(plan, m.dtype, nrhs, elem_off * m.element_size() + m.data_ptr(), lds,
                                         plan._pointers(rhs, nrhs, stream), None, plan._pointers(out, nrhs, stream),
                                         None, status)

    # ---- Z = X R: applying stored inverses ----
    def resolved_apply_ragged(self, orders, nrhs: int, elem_bytes: int = 4):
        """The launches of one ``apply_pointers`` / ``apply_ragged`` / ``apply_diag_blocks`` call on members of these
        orders (each 1 ... 128) with ``nrhs`` columns, host only: a list of ``(first, count, lanes, chunk_cols)`` -- a
        range of the member list sorted by order, the lanes that own one member (8 / 16 / 32 / 64, or 128: one
        workgroup of 128 threads per member) and the columns the kernel holds at a time.  One launch per lane class
        that has members, at most five whatever ``nrhs`` is.  An order outside 1 ... 128, ``nrhs < 1`` or an
        ``elem_bytes`` other than 4 or 8 raises ValueError."""
        o, size = _order_array(orders)
        count = ctypes.c_int()
        out = np.empty((5, 4), np.int32)
        _lib.check(self._lib.mi32_vbatch_apply_launches(_int_ptr(o), size, int(nrhs), int(elem_bytes), _int_ptr(out), 5,
                                                        ctypes.byref(count)), "mi32_vbatch_apply_launches")
        return [tuple(int(v) for v in row) for row in out[:count.value]]

    def apply_pointers(self, plan, x_ptrs, r_ptrs, z_ptrs, dtype, nrhs, ldx=None, ldr=None, ldz=None):
        """``Z_b = X_b R_b`` for every member of the plan in one call, the low-level form: ``x_ptrs`` / ``r_ptrs`` /
        ``z_ptrs`` are int64 device tensors of ``plan.batch`` member addresses (row-major members of ``dtype`` float32
        / float64: X is n x n, R and Z are n x ``nrhs``), ``ldx`` / ``ldr`` / ``ldz`` int32 device tensors of leading
        dimensions in elements (None: the member's order for ``ldx``, ``nrhs`` for the other two).  Every component is
        one chain of fused multiply-adds over j ascending from +0, so the result is reproducible bit for bit; there
        is no status.  A member may be applied in place (the same address and leading dimension for R and Z); Z over
        X, or members that overlap otherwise, are undefined.  Asynchronous on torch's current stream."""
        check_pointer_args(self.device, plan, dtype, {"x_ptrs": x_ptrs, "r_ptrs": r_ptrs, "z_ptrs": z_ptrs},
                           {"ldx": ldx, "ldr": ldr, "ldz": ldz}, nrhs=nrhs, want_status=False)
        self._bind_stream()
        self._apply_vbatched(plan, dtype, nrhs, x_ptrs, ldx, r_ptrs, ldr, z_ptrs, ldz)

    def _apply_vbatched(self, plan, dtype, nrhs, x_ptrs, ldx, r_ptrs, ldr, z_ptrs, ldz):
        """The library call of the variable-size applications, on the stream bound."""
        _lib.check(self._entry("mi32_apply_device_vbatched", dtype)(
            self._h, plan._p, _ptr(x_ptrs), _ptr(ldx), _ptr(r_ptrs), _ptr(ldr), int(nrhs), _ptr(z_ptrs), _ptr(ldz)),
            "mi32_apply_device_vbatched")

    def apply_ragged(self, plan, x_flat, r, out=None):
        """``z = blockdiag(X) r`` for members of mixed orders 1 ... 128 in one call: with ``x_flat`` the inverses
        ``inv_ragged`` stored, the application of a block-Jacobi preconditioner at n^2 multiply-adds per block.
        ``x_flat`` is the packed layout of ``inv_ragged``; ``r`` is a contiguous ``(plan.total_rows,)`` or
        ``(plan.total_rows, K)`` tensor of x_flat's dtype and device in which member i's rows start at
        ``sum_{k<i} n_k`` (a vector keeps its shape).  ``out`` may be ``r`` itself (in place) or a contiguous tensor
        of its shape that meets r's memory nowhere; it never meets that of ``x_flat``.  Returns z."""
        check_packed_matrices(self.device, plan, x_flat, "x_flat", want_status=False)
        rhs, out, nrhs = check_packed_rhs(plan, x_flat, r, out, "r")
        stream = self._bind_stream()
        self._apply_vbatched(plan, x_flat.dtype, nrhs, plan._pointers(x_flat, None, stream), None,
                             plan._pointers(rhs, nrhs, stream), None, plan._pointers(out, nrhs, stream), None)
        return out

    def apply_diag_blocks(self, x, block_orders, r, out=None):
        """``z = blockdiag(x) r`` in one call: ``x`` holds the consecutive diagonal blocks of the orders
        ``block_orders`` (each 1 ... 128, summing to N) either as the dense square N x N matrix ``inv_diag_blocks``
        returns, of which only the block entries are read, or as a 1-D packed tensor (``inv_diag_blocks(...,
        packed=True)``).  ``r`` is ``(N,)`` or ``(N, K)`` of x's dtype and device; ``out`` as in ``apply_ragged``.
        Returns z.  The plan of the last block structure is kept (shared with ``inv_diag_blocks``)."""
        if x.dim() == 1:
            return self.apply_ragged(self._diag_blocks_plan(None, block_orders)[0], x, r, out)
        plan, elem_off, lds = self._diag_blocks_plan(x, block_orders)
        check_ragged_call(self.device, plan, x.dtype, want_status=False)
        rhs, out, nrhs = check_packed_rhs(plan, x, r, out, "r")
        stream = self._bind_stream()
        self._apply_vbatched(plan, x.dtype, nrhs, elem_off * x.element_size() + x.data_ptr(), lds,
                             plan._pointers(rhs, nrhs, stream), None, plan._pointers(out, nrhs, stream), None)
        return out

    def _diag_blocks_plan(self, m, block_orders):
        """``(plan, element offsets of the blocks in m, leading dimensions)`` for the diagonal blocks of ``m``
        (``check_diag_blocks``; None: the packed form), from the one-entry cache ``_diag_plan`` where the block
        structure is that of the last call."""
        torch = self._torch
        orders = check_diag_blocks(self.device, m, block_orders)
        ld = int(orders.sum())
        key = orders.astype(np.int32).tobytes()
        if self._diag_plan is None or self._diag_plan[0] != key:
            if self._diag_plan is not None:
                self._diag_plan[1].close()
            plan = self.plan_ragged(orders)
            off = np.concatenate(([0], np.cumsum(orders.astype(np.int64))[:-1]))
            # block b starts at row off_b, column off_b: element off_b * (ld + 1)
            self._diag_plan = (key, plan, torch.from_numpy(off * (ld + 1)).to(self.device),
                               torch.full((orders.size,), ld, dtype=torch.int32, device=self.device))
        return self._diag_plan[1:]

    def inv_diag_blocks(self, m, block_orders, out=None, *, det=False, packed=False):
        """Invert the consecutive diagonal blocks of the square device matrix ``m`` (the block-Jacobi case): their
        orders (each 1 ... 128) must sum to ``m.shape[0]``.  Only the block entries of ``out`` (same shape, zeros by
        default; ``m`` itself, or memory that meets m's nowhere) are written, and only the block entries of ``m`` are
        read.  Returns ``(out, status)``; with ``det=True`` ``(out, status, (det_mant, det_exp))``, one pair per block
        (the determinant of the block-diagonal matrix is their product: add the logarithms of ``slogdet_from_frexp``).
        ``packed=True``: ``out`` is the packed layout of ``inv_ragged`` instead -- a 1-D tensor of ``sum n_b^2``
        elements, block b at offset ``sum_{i<b} n_i^2``, what ``apply_diag_blocks`` takes -- and no N x N buffer is
        touched."""
        plan, elem_off, lds = self._diag_blocks_plan(m, block_orders)
        status = check_ragged_call(self.device, plan, m.dtype)
        out = check_inverse_out(m, out, (plan.flat_size,) if packed else m.shape, zero=not packed)
        stream = self._bind_stream()
        if packed:
            out_ptrs, ldout = plan._pointers(out, None, stream), None
        else:
            out_ptrs, ldout = elem_off * out.element_size() + out.data_ptr(), lds
        r = self._inv_vbatched(plan, m.dtype, elem_off * m.element_size() + m.data_ptr(), lds, out_ptrs, ldout, status,
                               det)
        return (out, r[0], r[1]) if det else (out, r)

    # ---- from a sparse matrix: the blocks of a CSR matrix, gathered on the device ----
    def csr_diag_blocks(self, a, block_orders, out=None, *, first_rows=None, validate=False):
        """The square diagonal blocks of a sparse matrix in the packed layout of ``inv_ragged``, gathered on the device
        in one call (at most five launches) without a dense N x N copy.  ``a`` is a 2-D square ``torch.sparse_csr``
        tensor or a ``(crow, col, values)`` triple (``check_csr``: int32 or int64 indices, float32 or float64 values);
        ``block_orders`` as in ``inv_diag_blocks``, each 1 ... 128.  Without ``first_rows`` the blocks are consecutive
        and the orders sum to N; ``first_rows``, a host integer sequence with one entry per block, puts block b at
        rows and columns ``first_rows[b] ... first_rows[b] + n_b - 1`` instead: blocks may overlap or skip rows.
        Element (i, j) of a block is the stored value copied bit for bit, ``+0.0`` where none is stored; columns need
        no order inside a row; a (row, column) pair stored twice is the caller's error.  ``out``: a contiguous 1-D
        tensor of ``sum n_b^2`` elements of values' dtype and device that meets ``values`` nowhere.
        ``validate=True`` adds the synchronising checks of ``validate_csr``; the default path does not synchronise.
        Asynchronous on torch's current stream.  Returns the packed tensor; the plan of the last block structure is
        kept (shared with ``inv_diag_blocks``)."""
        crow, col, values = csr_parts(a)
        n = check_csr(self.device, crow, col, values)
        orders = check_diag_blocks(self.device, None, block_orders)
        first = check_csr_first_rows(first_rows, orders, n)
        plan = self._diag_blocks_plan(None, orders)[0]
        check_ragged_call(self.device, plan, values.dtype, want_status=False)
        out = check_csr_out(values, out, plan.flat_size)
        if validate:
            validate_csr(crow, col, n)
        # the consecutive first rows are the plan's row offsets, already on the device
        d_first = plan._row_offsets if first_rows is None else self._torch.from_numpy(first).to(self.device)
        stream = self._bind_stream()
        _lib.check(self._entry("mi32_csr_blocks_device", values.dtype)(
            self._h, plan._p, _ptr(crow), _ptr(col), crow.element_size(), _ptr(values), _ptr(d_first),
            _ptr(plan._pointers(out, None, stream)), None), "mi32_csr_blocks_device")
        return out

    def inv_csr_blocks(self, a, block_orders, *, first_rows=None, det=False, validate=False):
        """Block-Jacobi set-up from the sparse matrix: ``csr_diag_blocks``, then ``inv_ragged`` in place on the same
        stream.  Returns ``(x_packed, status)``, or ``(x_packed, status, (det_mant, det_exp))`` with ``det=True`` --
        what ``inv_diag_blocks(dense, block_orders, packed=True)`` returns for the dense form of ``a``, and what
        ``apply_diag_blocks(x_packed, block_orders, r)`` takes as it is."""
        x = self.csr_diag_blocks(a, block_orders, first_rows=first_rows, validate=validate)
        return self.inv_ragged(self._diag_blocks_plan(None, block_orders)[0], x, out=x, det=det)

    # ---- the block structure itself, from the sparsity pattern ----
    def csr_block_starts(self, a, max_order=32, *, agglomerate=True, out=None):
        """Where the block-Jacobi blocks of a sparse matrix begin, found on the device from its sparsity pattern by
        supervariable agglomeration: a uint8 device tensor of N entries, 1 at the first row of every block.  ``a`` as in
        ``csr_diag_blocks``, or a ``(crow, col, None)`` triple: the values are not read.  Consecutive rows with the same
        column indices IN STORED ORDER form a supervariable, cut every ``max_order`` (1 ... 128) rows; with
        ``agglomerate`` consecutive supervariables are merged while their rows sum to at most ``max_order``.  Rows
        that hold the same set in a different order count as different: sort unsorted rows first (``torch``'s CSR
        tensors are sorted).  ``out``: a contiguous uint8 tensor of N entries on the device that meets ``crow`` and
        ``col`` nowhere.  The temporary memory (2.1 bytes per row) is a ``torch.empty`` of this call.  Asynchronous on
        torch's current stream; no synchronisation."""
        torch = self._torch
        crow, col = csr_pattern_parts(a)
        n = check_csr_pattern(self.device, crow, col)
        max_order, agglomerate = check_find_blocks_args(max_order, agglomerate)
        out = check_block_starts_out(crow, col, out, n)
        nbytes = find_blocks_work_bytes(n)
        work = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self._bind_stream()
        # (a pattern without entries has no col to point at: every row is empty and no entry is read, crow stands in)
        _lib.check(self._lib.mi32_csr_find_blocks_device(
            self._h, n, _ptr(crow), _ptr(col if col.numel() else crow), crow.element_size(), max_order,
            int(agglomerate), _ptr(out), _ptr(work), nbytes), "mi32_csr_find_blocks_device")
        return out

    def csr_find_blocks(self, a, max_order=32, *, agglomerate=True):
        """The block orders of ``csr_block_starts`` as a host ``np.int32`` array, what every ``block_orders=`` argument
        takes: they sum to N and each is in 1 ... ``max_order``.  One N-byte copy to the host (this synchronises);
        plans are binned on the host, so the orders have to arrive there in any case."""
        start = self.csr_block_starts(a, max_order, agglomerate=agglomerate).cpu().numpy()
        first = np.flatnonzero(start)
        return np.diff(first, append=start.size).astype(np.int32)

    # ---- block inverses stored in reduced precision per block, and applied from that store ----
    def _block_stats(self, plan, dtype, ptrs, ld):
        """The library call of the block statistics, on the stream bound."""
        stats = self._torch.empty((plan.batch, 3), dtype=self._torch.float64, device=self.device)
        _lib.check(self._entry("mi32_block_stats_device", dtype)(self._h, plan._p, _ptr(ptrs), _ptr(ld), _ptr(stats)),
                   "mi32_block_stats_device")
        return stats

    def block_stats(self, plan, flat):
        """``(norm1, absmax, absmin)`` of every member of the packed tensor ``flat`` (the layout of ``inv_ragged``) as
        a float64 ``(plan.batch, 3)`` device tensor in the caller's member order: the 1-norm (column sums of magnitudes
        added in float64, rows ascending), the largest magnitude and the smallest nonzero one (``+inf`` for an all-zero
        member).  A member with a NaN entry gives three NaNs.  One call, at most five launches, asynchronous on
        torch's current stream."""
        check_packed_matrices(self.device, plan, flat, "flat", want_status=False)
        stream = self._bind_stream()
        return self._block_stats(plan, flat.dtype, plan._pointers(flat, None, stream), None)

    def block_stats_pointers(self, plan, ptrs, dtype, ld=None):
        """``block_stats`` in the low-level form: ``ptrs`` is an int64 device tensor of ``plan.batch`` member addresses
        (row-major members of ``dtype``), ``ld`` an int32 device tensor of leading dimensions (None: the orders).
        Padding behind a row is never read."""
        check_pointer_args(self.device, plan, dtype, {"ptrs": ptrs}, {"ld": ld}, want_status=False)
        self._bind_stream()
        return self._block_stats(plan, dtype, ptrs, ld)

    def _store(self, plan, dtype, x_ptrs, ldx, formats, layout, data):
        """The library call of the store kernels, on the stream bound: ``formats`` is the checked host array,
        ``layout`` its ``stored_layout``, ``data`` the checked buffer or None for a new one."""
        torch = self._torch
        offsets, nbytes = layout
        if data is None:
            data = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        d_formats = torch.from_numpy(formats).to(self.device)
        d_offsets = torch.from_numpy(offsets).to(self.device)
        _lib.check(self._entry("mi32_store_inverses_device", dtype)(
            self._h, plan._p, _ptr(x_ptrs), _ptr(ldx), _ptr(d_formats), _ptr(d_offsets), _ptr(data)),
            "mi32_store_inverses_device")
        counts = tuple(int(c) for c in np.bincount(formats, minlength=len(STORAGE_FORMATS)))
        native = torch.empty(0, dtype=dtype).element_size()
        return StoredInverses(plan, dtype, d_formats, d_offsets, data, nbytes, plan.flat_size * native, counts)

    def _store_layout(self, plan, dtype, formats, data, x_flat=None):
        """``(checked host formats, stored_layout)`` of a store call, and the check of a caller's ``data``."""
        f = check_storage_formats(plan, dtype, formats)
        layout = stored_layout(plan.orders, f, self._torch.empty(0, dtype=dtype).element_size())
        if data is not None:
            check_store_data(self.device, data, layout[1], x_flat)
        return f, layout

    def store_inverses(self, plan, x_flat, formats, *, data=None):
        """Narrow every member of the packed tensor ``x_flat`` (what ``inv_ragged`` returns) to its own storage format
        and return the ``StoredInverses`` that ``apply_stored`` reads.  ``formats``: one code of ``STORAGE_FORMATS``
        per member, a host integer sequence or a device int32 tensor (``choose_storage`` returns one); code 1 (float32)
        is for float64 members only.  The codes are checked on the host and the buffer is sized from them: with a
        device tensor this is the one synchronisation of the set-up.  Narrowing is round-to-nearest-even with IEEE
        results, from float64 to a 16-bit format through float32.  ``data``: a uint8 device tensor to store into
        instead of a new one (at least the store's size, 8-byte aligned, away from ``x_flat``); bytes between members
        are never written.  ``x_flat`` is not kept.  One call, at most five launches."""
        check_packed_matrices(self.device, plan, x_flat, "x_flat", want_status=False)
        f, layout = self._store_layout(plan, x_flat.dtype, formats, data, x_flat)
        stream = self._bind_stream()
        return self._store(plan, x_flat.dtype, plan._pointers(x_flat, None, stream), None, f, layout, data)

    def store_inverses_pointers(self, plan, x_ptrs, dtype, formats, ldx=None, *, data=None):
        """``store_inverses`` in the low-level form: ``x_ptrs`` is an int64 device tensor of ``plan.batch`` member
        addresses (row-major members of ``dtype``), ``ldx`` an int32 device tensor of leading dimensions (None: the
        orders).  The store itself is always dense."""
        check_pointer_args(self.device, plan, dtype, {"x_ptrs": x_ptrs}, {"ldx": ldx}, want_status=False)
        f, layout = self._store_layout(plan, dtype, formats, data)
        self._bind_stream()
        return self._store(plan, dtype, x_ptrs, ldx, f, layout, data)

    def _apply_stored(self, stored, nrhs, r_ptrs, ldr, z_ptrs, ldz):
        """The library call of the applications from a store, on the stream bound."""
        _lib.check(self._entry("mi32_apply_stored_device", stored.dtype)(
            self._h, stored.plan._p, _ptr(stored.data), _ptr(stored.offsets), _ptr(stored.formats), _ptr(r_ptrs),
            _ptr(ldr), int(nrhs), _ptr(z_ptrs), _ptr(ldz)), "mi32_apply_stored_device")

    def apply_stored(self, stored, r, out=None):
        """``z = blockdiag(widen(X)) r`` from a ``StoredInverses``: the call of ``apply_ragged`` with every member read
        in its storage format (2, 4 or 8 bytes per element) and widened exactly on the way into the multiply-adds,
        which are unchanged -- the result has the bits of ``apply_ragged`` on the widened members.  ``r`` and ``out``
        as in ``apply_ragged`` (``out`` may be ``r``; it must not meet ``stored.data``).  Returns z."""
        if not isinstance(stored, StoredInverses):
            raise ValueError("expected the StoredInverses of store_inverses")
        plan = stored.plan
        check_ragged_call(self.device, plan, stored.dtype, want_status=False)
        rhs, out, nrhs = check_packed_rhs(plan, _StoreSpan(stored.dtype, stored.data), r, out, "r")
        stream = self._bind_stream()
        self._apply_stored(stored, nrhs, plan._pointers(rhs, nrhs, stream), None, plan._pointers(out, nrhs, stream), None)
        return out

    def apply_stored_pointers(self, stored, r_ptrs, z_ptrs, nrhs, ldr=None, ldz=None):
        """``apply_stored`` in the low-level form of ``apply_pointers``: ``r_ptrs`` / ``z_ptrs`` are int64 device
        tensors of member addresses (R and Z are n x ``nrhs``, row-major in ``stored.dtype``), ``ldr`` / ``ldz`` int32
        device tensors of leading dimensions (None: ``nrhs``).  A member may be applied in place; what the addresses
        point to cannot be checked."""
        if not isinstance(stored, StoredInverses):
            raise ValueError("expected the StoredInverses of store_inverses")
        check_pointer_args(self.device, stored.plan, stored.dtype, {"r_ptrs": r_ptrs, "z_ptrs": z_ptrs},
                           {"ldr": ldr, "ldz": ldz}, nrhs=nrhs, want_status=False)
        self._bind_stream()
        self._apply_stored(stored, nrhs, r_ptrs, ldr, z_ptrs, ldz)

    def inv_csr_blocks_adaptive(self, a, block_orders, *, tol=0.1, first_rows=None, validate=False):
        """Adaptive-precision block-Jacobi set-up from the sparse matrix, on one stream: ``csr_diag_blocks``,
        ``block_stats`` of the blocks, ``inv_ragged`` in place, ``block_stats`` of the inverses, ``choose_storage``
        with ``kappa = norm1(A) * norm1(X)``, the inversion's status and ``tol``, and ``store_inverses``.  Returns
        ``(stored, status, formats)``: the ``StoredInverses`` for ``apply_stored``, one status word per block and the
        chosen format codes (int32, device).  A block whose status is not 0 is stored native, as the inversion left
        it.  Synchronises once, to size the store.  The plan goes with the result (``stored.plan``): it is taken out of
        the Inverter's one-entry cache."""
        x = self.csr_diag_blocks(a, block_orders, first_rows=first_rows, validate=validate)
        plan = self._diag_blocks_plan(None, block_orders)[0]
        stats_a = self.block_stats(plan, x)
        x, status = self.inv_ragged(plan, x, out=x)
        stats_x = self.block_stats(plan, x)
        formats = choose_storage(x.dtype, stats_a[:, 0] * stats_x[:, 0], stats_x[:, 1].contiguous(),
                                 stats_x[:, 2].contiguous(), tol, status)
        stored = self.store_inverses(plan, x, formats)
        self._diag_plan = None  # the stored object owns the plan now
        return stored, status, formats

    # ---- a solver-level use of the store: the residual of the block rows, and the fused block-Jacobi sweep ----
    def csr_block_residual(self, a, plan, x, b, out=None, *, first_rows=None, validate=False):
        """``r = (b - A x)`` at the rows of the blocks, in the packed layout that ``apply_stored`` and ``apply_ragged``
        take (member i's rows start at ``sum_{k<i} n_k``), in one call (at most five launches).  ``a`` as in
        ``csr_diag_blocks``; ``plan`` is the RaggedPlan of the block orders; ``first_rows`` as in ``csr_diag_blocks``
        (None: consecutive blocks whose orders sum to N; blocks may overlap or skip rows).  ``x`` and ``b`` are
        contiguous N-vectors of values' dtype and device.  The arithmetic is fixed bit for bit: per row eight partial
        sums over the stored entries in stored order, ``p[e % 8] = fma(val_e, x[col_e], p[e % 8])``, a three-level
        butterfly ``(p_s + p_{s^4}) + (.. s^2) + (.. s^1)`` and ``b - sum``, whatever the block order or the index
        dtype.  ``out``: a contiguous 1-D tensor of ``plan.total_rows`` entries that meets neither ``x``, ``b`` nor
        the CSR arrays.  ``validate=True`` adds the synchronising checks of ``validate_csr``.  Asynchronous on
        torch's current stream.  Returns r."""
        crow, col, values = csr_parts(a)
        n = check_csr(self.device, crow, col, values)
        check_ragged_call(self.device, plan, values.dtype, want_status=False)
        first = check_csr_first_rows(first_rows, plan.orders, n)
        check_relax_vectors(values, n, x, b)
        out = check_relax_out(values, out, plan.total_rows, {"x": x, "b": b, "crow": crow, "col": col, "values": values})
        if validate:
            validate_csr(crow, col, n)
        if out is None:
            out = self._torch.empty(plan.total_rows, dtype=values.dtype, device=values.device)
        d_first = plan._row_offsets if first_rows is None else self._torch.from_numpy(first).to(self.device)
        stream = self._bind_stream()
        _lib.check(self._entry("mi32_csr_block_residual_device", values.dtype)(
            self._h, plan._p, _ptr(crow), _ptr(col), crow.element_size(), _ptr(values), _ptr(d_first), _ptr(x), _ptr(b),
            _ptr(plan._pointers(out, 1, stream))), "mi32_csr_block_residual_device")
        return out

    def relax_stored(self, a, stored, x, b, omega=1.0, out=None, *, first_rows=None, sweeps=1, validate=False):
        """Block-Jacobi relaxation from the sparse matrix and the stored block inverses, fused:
        ``x' = x + omega * blockdiag(A)^-1 (b - A x)`` in one call per sweep (at most five launches; the residual
        never goes to memory).  ``a`` as in ``csr_diag_blocks``; ``stored`` is the ``StoredInverses`` of the blocks
        (``inv_csr_blocks_adaptive`` or ``store_inverses``), of the matrix's dtype; ``first_rows`` places its members
        as in ``csr_diag_blocks``, and the blocks must not overlap one another.  Bit for bit,
        ``x'[rows of block b] = fma(omega, z_b, x[rows of block b])`` with ``z_b`` what ``apply_stored`` returns on
        ``csr_block_residual``'s r.  Rows in no block are not written: ``out=None`` gives a new tensor where the
        blocks tile ``[0, N)`` and ``x.clone()`` otherwise.  ``out``: a contiguous N-vector that meets neither ``x``,
        ``b``, the CSR arrays nor ``stored.data`` (every block reads the old x).  ``sweeps=k`` runs k sweeps on the
        stream, ping-ponging between ``out`` and one temporary, with no host synchronisation; where the blocks do not
        tile ``[0, N)``, the rows in no block are the fixed part of the iterate, and with ``k > 1`` a given ``out``
        first receives them from ``x``.  Asynchronous on torch's current stream.  Returns x'."""
        if not isinstance(stored, StoredInverses):
            raise ValueError("expected the StoredInverses of store_inverses")
        crow, col, values = csr_parts(a)
        n = check_csr(self.device, crow, col, values)
        if stored.dtype != values.dtype:
            raise ValueError(f"stored holds {stored.dtype} members, the matrix is {values.dtype}")
        plan = stored.plan
        check_ragged_call(self.device, plan, stored.dtype, want_status=False)
        sweeps, omega = check_sweeps(sweeps, omega)
        first = check_csr_first_rows(first_rows, plan.orders, n)
        check_blocks_disjoint(first, plan.orders)
        check_relax_vectors(values, n, x, b)
        out = check_relax_out(values, out, n, {"x": x, "b": b, "crow": crow, "col": col, "values": values,
                                                 "stored.data": stored.data})
        if validate:
            validate_csr(crow, col, n)
        tiles = plan.total_rows == n  # disjoint blocks inside the matrix: they cover it where their rows are all of it
        if out is None:
            out = self._torch.empty_like(x) if tiles else x.clone()
        elif not tiles and sweeps > 1:
            out.copy_(x)
        tmp = None
        if sweeps > 1:
            tmp = self._torch.empty_like(x) if tiles else x.clone()
        d_first = plan._row_offsets if first_rows is None else self._torch.from_numpy(first).to(self.device)
        fn = self._entry("mi32_csr_relax_stored_device", values.dtype)
        self._bind_stream()
        src = x
        for j in range(sweeps):
            dst = out if (sweeps - 1 - j) % 2 == 0 else tmp
            _lib.check(fn(self._h, plan._p, _ptr(crow), _ptr(col), crow.element_size(), _ptr(values), _ptr(d_first),
                          _ptr(stored.data), _ptr(stored.offsets), _ptr(stored.formats), _ptr(src), _ptr(b), omega,
                          _ptr(dst)), "mi32_csr_relax_stored_device")
            src = dst
        return out

    def set_lookahead(self, enable: bool):
        _lib.check(self._lib.mi32_set_lookahead(self._h, 1 if enable else 0), "mi32_set_lookahead")

    def set_profiling(self, enable: bool):
        _lib.check(self._lib.mi32_set_profiling(self._h, 1 if enable else 0), "mi32_set_profiling")

    def get_profile(self):
        """{class: (milliseconds, launches)} since the last call (synchronises the recorded events)."""
        k = len(_lib.KERNEL_CLASSES)
        ms = (ctypes.c_double * k)()
        cnt = (ctypes.c_longlong * k)()
        _lib.check(self._lib.mi32_get_profile(self._h, ms, cnt, k), "mi32_get_profile")
        return {name: (ms[i], int(cnt[i])) for i, name in enumerate(_lib.KERNEL_CLASSES)}

    def residual(self, a, x):
        """Device-side check: returns a (B,3) float64 tensor [||AX-I||_inf, ||XA-I||_inf, sqrt(N)-||AX||_F].
        a, x: float32 tensors on this device of one shape, (N,N) or (B,N,N), any B; anything else raises ValueError.
        A member with a NaN entry gives NaN in its three outputs; the other members are not affected."""
        torch = self._torch
        for t, what in ((a, "a"), (x, "x")):
            if t.dtype != torch.float32 or not t.is_cuda:
                raise ValueError(f"{what}: expected a float32 tensor on the GPU")
            if t.device != self.device:
                raise ValueError(f"{what} is on {t.device}, expected {self.device}")
        a3 = (a.unsqueeze(0) if a.dim() == 2 else a).contiguous()
        x3 = (x.unsqueeze(0) if x.dim() == 2 else x).contiguous()
        if a3.dim() != 3 or a3.shape[1] != a3.shape[2] or a3.shape[0] == 0 or a3.shape[1] == 0:
            raise ValueError("expected (N,N) or (B,N,N)")
        if x3.shape != a3.shape:
            raise ValueError(f"x has shape {tuple(x.shape)}, a {tuple(a.shape)}")
        b, n = a3.shape[0], a3.shape[1]
        out = torch.empty(b, 3, dtype=torch.float64, device=a3.device)
        self._bind_stream()
        _lib.check(self._lib.mi32_residual_device(self._h, ctypes.c_void_p(a3.data_ptr()),
                                                  ctypes.c_void_p(x3.data_ptr()), n, b,
                                                  ctypes.c_void_p(out.data_ptr())), "mi32_residual_device")
        return out
