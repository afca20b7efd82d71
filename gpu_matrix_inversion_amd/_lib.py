"""ctypes binding of ``lib/libmat_inv_32.so`` (the C ABI of include/mat_inv_32_c.h).

This is the binding a maintainer of the reference would write to call the
HIP library from Python.  There is deliberately no CPU
fallback: if the shared library is missing or cannot be loaded, every entry
point raises.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmat_inv_32.so")
CSRC_DIR = os.path.join(_HERE, "csrc")

MI32_OK = 0
MI32_BAD_SHAPE = 1
MI32_SINGULAR = 2
MI32_RUNTIME_ERROR = 3

ALGO_AUTO = 0
ALGO_SWEEP = 1
ALGO_BLOCKED = 2
ALGO_RESIDENT = 3
ALGO_WORKGROUP = 4
ALGO_WIDE = 5
ALGO_NAMES = {"auto": ALGO_AUTO, "sweep": ALGO_SWEEP, "blocked": ALGO_BLOCKED, "resident": ALGO_RESIDENT,
              "workgroup": ALGO_WORKGROUP, "wide": ALGO_WIDE}
# the eight kernel classes of a variable-size batch: the largest order each takes (mi32_vbatch_bin)
VBATCH_CLASS_TOPS = (8, 16, 32, 64, 80, 96, 112, 128)
KERNEL_CLASSES = ("init", "sweep_step", "panel", "update_in_block", "update_rank_bw", "finish", "panel_transpose")

# the C++ drop-in of include/mat_inv_32.h (Itanium-mangled matrix_inv_32(std::vector<float>, int))
CXX_DROPIN_SYMBOL = "_Z13matrix_inv_32St6vectorIfSaIfEEi"
# the fp64 twin of include/mat_inv_64.h: matrix_inversion_FP64(std::vector<double>, int)
CXX_FP64_SYMBOL = "_Z21matrix_inversion_FP64St6vectorIdSaIdEEi"
# the no-pivot variant of include/mat_inv_64.h: matrix_inversion_no_pivots(std::vector<double>, int)
CXX_NOPIVOT_SYMBOL = "_Z26matrix_inversion_no_pivotsSt6vectorIdSaIdEEi"
# the benchmark twin of include/mat_inv_bench.h: Res FP32_bench(std::vector<float>, int)
CXX_BENCH_SYMBOL = "_Z10FP32_benchSt6vectorIfSaIfEEi"
TIMES10_SLOTS = ("queue", "buffers", "build", "makeAug", "pivot", "row", "column", "compute", "getInverted", "total")


class Mi32Error(RuntimeError):
    pass


class Route(ctypes.Structure):
    """mi32_route_t: how a blocked fp32 call runs (mi32_resolve_route)."""
    _fields_ = [("np", ctypes.c_int), ("block_width", ctypes.c_int), ("nblocks", ctypes.c_int),
                ("shared_panels", ctypes.c_int), ("lookahead", ctypes.c_int), ("parts", ctypes.c_int),
                ("part_batch", ctypes.c_int * 2), ("part_strips_at_end", ctypes.c_int * 2),
                ("first_fused_block", ctypes.c_int)]


_I, _Z, _VP = ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p
_IP, _FP, _DP = ctypes.POINTER(_I), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)


def _signatures(*rows):
    """{symbol: (restype, argtypes)} from rows of ("name [name ...]", restype, argtypes): the names of one row (an
    entry point and its twins) share the signature."""
    return {name: (restype, argtypes) for names, restype, argtypes in rows for name in names.split()}


# every symbol include/mat_inv_32_c.h declares, in the header's parameter order, and the two debug hooks load() binds
SIGNATURES = _signatures(
    ("mi32_matrix_inv_32", _I, [_FP, _Z, _I, _FP]),
    ("mi32_matrix_inv_32_batched", _I, [_FP, _I, _I, _FP, _IP]),
    ("mi32_matrix_inv_32_batched_multi", _I, [_FP, _I, _I, _FP, _IP, _I]),
    ("mi32_shard_range", _I, [_I, _I, _I, _IP, _IP]),
    ("mi32_create", _I, [ctypes.POINTER(_VP), _I]),
    ("mi32_destroy mi32_vbatch_destroy", _I, [_VP]),
    ("mi32_set_stream", _I, [_VP, _VP]),
    ("mi32_set_algo mi32_set_lookahead mi32_set_profiling mi32_set_pivoting", _I, [_VP, _I]),
    ("mi32_set_blocking mi32_reserve mi32_resolve_algo", _I, [_VP, _I, _I]),
    ("mi32_workspace_bytes", _Z, [_I, _I, _I]),
    ("mi32_inv_device mi32_inv_device_f64", _I, [_VP, _VP, _I, _I, _VP, _VP]),
    ("mi32_residual_device", _I, [_VP, _VP, _VP, _I, _I, _VP]),
    ("mi32_get_profile", _I, [_VP, _DP, ctypes.POINTER(ctypes.c_longlong), _I]),
    ("mi32_last_timing", _I, [_DP, _DP]),
    ("mi32_bench_32", _I, [_FP, _Z, _I, _FP, _DP]),
    ("mi32_bench_64", _I, [_DP, _Z, _I, _DP, _DP, _I]),
    ("mi32_matrix_multiply_64", _I, [_DP, _DP, _Z, _DP]),
    ("mi32_matrix_inv_64 mi32_matrix_inversion_no_pivots", _I, [_DP, _Z, _I, _DP]),
    ("mi32_resolve_blocking_f64", _I, [_VP, _I, _IP]),
    ("mi32_resolve_blocking mi32_resolve_resident", _I, [_VP, _I, _I, _IP, _IP]),
    ("mi32_resolve_workgroup mi32_resolve_wide", _I, [_VP, _I, _I, _IP, _IP, _IP]),
    ("mi32_resolve_panel_widths", _I, [_VP, _I, _I, _IP, _I, _IP]),
    ("mi32_resolve_route", _I, [_VP, _I, _I, ctypes.POINTER(Route), _IP, _I]),
    ("mi32_vbatch_bin", _I, [_IP, _I, _IP, _IP]),
    ("mi32_vbatch_create", _I, [_VP, _IP, _I, ctypes.POINTER(_VP)]),
    ("mi32_vbatch_info", _I, [_VP, _IP, _IP]),
    ("mi32_inv_device_vbatched mi32_inv_device_vbatched_f64", _I, [_VP] * 7),
    ("mi32_inv_det_device mi32_inv_det_device_f64 mi32_inv_det_any_device mi32_inv_det_any_device_f64", _I,
     [_VP, _VP, _I, _I, _VP, _VP, _VP, _VP]),
    ("mi32_inv_det_device_vbatched mi32_inv_det_device_vbatched_f64", _I, [_VP] * 9),
    ("mi32_solve_device mi32_solve_device_f64", _I, [_VP, _VP, _I, _I, _VP, _I, _VP, _VP]),
    ("mi32_resolve_solve", _I, [_VP, _I, _I, _I, _IP, _IP, _IP, _IP]),
    ("mi32_solve_device_vbatched mi32_solve_device_vbatched_f64", _I, [_VP] * 6 + [_I] + [_VP] * 3),
    ("mi32_vbatch_solve_launches", _I, [_IP, _I, _I, _IP, _I, _IP]),
    ("mi32_apply_device_vbatched mi32_apply_device_vbatched_f64", _I, [_VP] * 6 + [_I] + [_VP] * 2),
    ("mi32_vbatch_apply_launches", _I, [_IP, _I, _I, _I, _IP, _I, _IP]),
    ("mi32_dominant_kernel", ctypes.c_char_p, [_I]),
    ("mi32_last_error", ctypes.c_char_p, []),
    ("mi32_version", _I, []),
    ("mi32_debug_drop_panel_group", _I, [_I]),
    ("mi32_debug_dpp_selftest", _I, [_VP, _VP, _I, _VP]),
)
C_ABI_SYMBOLS = tuple(name for name in SIGNATURES if not name.startswith("mi32_debug_"))
# the sparse set-up calls, declared in a header of their own (include/mat_inv_32_csr.h)
CSR_SIGNATURES = _signatures(
    ("mi32_csr_blocks_device mi32_csr_blocks_device_f64", _I, [_VP] * 4 + [_I] + [_VP] * 4),
)
CSR_ABI_SYMBOLS = tuple(CSR_SIGNATURES)
# finding the blocks from the sparsity pattern, declared in a header of its own (include/mat_inv_32_csr_find.h), and the
# hook that runs its stages one by one (tools/csr_find_blocks_bench.py)
_LL = ctypes.c_longlong
_FIND_ARGS = [_VP, _LL, _VP, _VP, _I, _I, _I, _VP, _VP, _Z]
CSR_FIND_SIGNATURES = _signatures(
    ("mi32_csr_find_blocks_work_bytes", _I, [_LL, ctypes.POINTER(_Z)]),
    ("mi32_csr_find_blocks_device", _I, _FIND_ARGS),
    ("mi32_csr_find_blocks_chunk_rows", _I, []),
    ("mi32_debug_csr_find_stages", _I, _FIND_ARGS + [_I]),
)
CSR_FIND_ABI_SYMBOLS = tuple(name for name in CSR_FIND_SIGNATURES if not name.startswith("mi32_debug_"))
CSR_FIND_MAX_ORDER = 128
# block inverses stored in a per-member format, declared in a header of their own (include/mat_inv_32_stored.h)
STORED_SIGNATURES = _signatures(
    ("mi32_block_stats_device mi32_block_stats_device_f64", _I, [_VP] * 5),
    ("mi32_store_inverses_device mi32_store_inverses_device_f64", _I, [_VP] * 7),
    ("mi32_apply_stored_device mi32_apply_stored_device_f64", _I, [_VP] * 7 + [_I] + [_VP] * 2),
)
STORED_ABI_SYMBOLS = tuple(STORED_SIGNATURES)
# the block residual and the fused relaxation sweep, declared in a header of their own (include/mat_inv_32_relax.h);
# omega is passed by value in the working type
RELAX_SIGNATURES = _signatures(
    ("mi32_csr_block_residual_device mi32_csr_block_residual_device_f64", _I, [_VP] * 4 + [_I] + [_VP] * 5),
    ("mi32_csr_relax_stored_device", _I, [_VP] * 4 + [_I] + [_VP] * 7 + [ctypes.c_float, _VP]),
    ("mi32_csr_relax_stored_device_f64", _I, [_VP] * 4 + [_I] + [_VP] * 7 + [ctypes.c_double, _VP]),
)
RELAX_ABI_SYMBOLS = tuple(RELAX_SIGNATURES)


def build_library(force: bool = False) -> str:
    """Compile the HIP sources for gfx950 (hipcc cross-compiles without a GPU)."""
    if force and os.path.exists(LIB_PATH):
        os.remove(LIB_PATH)
    subprocess.check_call(["make", "-C", CSRC_DIR, "-s", "all"])
    if not os.path.exists(LIB_PATH):
        raise Mi32Error(f"build did not produce {LIB_PATH}")
    return LIB_PATH


_lib = None


def load() -> ctypes.CDLL:
    """Load the shared library; raises if it is absent (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise Mi32Error(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C gpu_matrix_inversion_amd/csrc`.  There is no CPU fallback."
        )
    try:
        # If torch is (or will be) in the process, its bundled HIP runtime must be the one this
        # library binds to (same SONAME libamdhip64.so.7), so that streams and device pointers are
        # shared: import torch first when it is importable.
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is optional for the pure ctypes/numpy path
        pass
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (restype, argtypes) in {**SIGNATURES, **CSR_SIGNATURES, **CSR_FIND_SIGNATURES, **STORED_SIGNATURES,
                                       **RELAX_SIGNATURES}.items():
        if name == "mi32_debug_dpp_selftest" and not hasattr(lib, name):
            continue  # tools/ab_bench.py also loads builds older than the self-test
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def resolve_route(handle, n: int, batch: int):
    """mi32_resolve_route as (dict of the mi32_route_t fields, workgroups per panel at the start of every outer block);
    ``handle`` may be None: what a fresh context does."""
    r = Route()
    groups = (ctypes.c_int * 128)()
    check(load().mi32_resolve_route(handle, int(n), int(batch), ctypes.byref(r), groups, 128), "mi32_resolve_route")
    route = {name: getattr(r, name) for name, _ in Route._fields_}
    route["part_batch"], route["part_strips_at_end"] = list(r.part_batch), list(r.part_strips_at_end)
    return route, [int(groups[b]) for b in range(r.nblocks)]


def check(rc: int, what: str) -> int:
    """Raise on MI32_RUNTIME_ERROR / MI32_BAD_SHAPE from a handle-level call."""
    if rc == MI32_RUNTIME_ERROR:
        raise Mi32Error(f"{what}: {load().mi32_last_error().decode()}")
    if rc == MI32_BAD_SHAPE:
        raise ValueError(f"{what}: bad shape or argument")
    return rc
