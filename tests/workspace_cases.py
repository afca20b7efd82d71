"""The workspace's diagnostic guard mode, as the tests see it: bindings of the tests-only entry points
(``mi32_debug_ws_guard`` / ``_layout`` / ``_check`` / ``_poke``, not part of include/mat_inv_32_c.h), the names the
documentation gives the regions, and the case tables of tests/test_gpu_workspace_guard.py.  Pure ctypes and numpy:
tests/test_workspace_layout.py uses the first half without a device.

The guard size ``G`` is process-wide, so every user goes through ``guard(lib, G)``, which puts it back to 0.
"""
import contextlib
import ctypes
from collections import namedtuple

import numpy as np

import guard_cases
import tall_batch_cases

F32, F64 = np.float32, np.float64
POISON = 0x7FF8DEAD          # a quiet NaN as a float; two of it are a quiet NaN as a double
POKE = 0xA5A5A5A5            # differs from the poison and from zero in every byte
G_HOST = 65536               # the guard size of the host-only layout tests
INVERSE, DET, RESIDUAL = 0, 1, 2      # WsCarve::Owner
VALUES, INDICES, RECORDS = 0, 1, 2    # mi32::WsKind
RESIDENT, WORKGROUP, SWEEP, BLOCKED32, BLOCKED64, NOPIVOT64, WIDE = range(7)  # DenseRoute::Path
ONE_LAUNCH = (RESIDENT, WORKGROUP, WIDE)

# DESIGN.md's region tables: the regions of each carve in order, and those that hold one slot per member
BLOCKED32_REGIONS = ("m0", "m1", "pt0", "pt1", "pt2", "gt0", "gt1", "mt0", "mt1", "aux0", "aux1", "xch", "gk", "ub0",
                     "xs0", "ub1", "xs1", "xst", "mf0", "mf1", "submap0", "submap1", "invsub0", "invsub1", "rowsrc0",
                     "rowsrc1", "rowsrc2", "rowsrc3", "orig", "invp")
REGIONS = {
    SWEEP: ("w0", "w1", "k0", "k1", "orig", "invp"),
    BLOCKED32: BLOCKED32_REGIONS,
    BLOCKED64: ("w0", "w1", "k0", "k1", "orig", "invp", "rowmap"),
    NOPIVOT64: ("w", "ft", "ub", "piv", "orig", "invp"),
}
DET_REGIONS = ("flag", "parity", "piv")
RESIDUAL_REGIONS = ("sums",)
PER_MEMBER = {"w0", "w1", "w", "ft", "ub", "m0", "m1", "pt0", "pt1", "pt2", "gt0", "gt1", "mt0", "mt1", "gk", "ub0",
              "xs0", "ub1", "xs1", "xst", "mf0", "mf1"}
KIND_OF = {name: VALUES for name in PER_MEMBER | {"aux0", "aux1", "piv", "sums"}}
KIND_OF.update({name: INDICES for name in ("orig", "invp", "rowmap", "submap0", "submap1", "invsub0", "invsub1",
                                           "rowsrc0", "rowsrc1", "rowsrc2", "rowsrc3")})
KIND_OF.update({name: RECORDS for name in ("k0", "k1", "xch", "flag", "parity")})


class Region(ctypes.Structure):  # mi32_debug_ws_region
    _fields_ = [("owner", ctypes.c_int), ("part", ctypes.c_int), ("kind", ctypes.c_int), ("reserved", ctypes.c_int),
                ("offset", ctypes.c_size_t), ("bytes", ctypes.c_size_t), ("name", ctypes.c_char * 16)]


class Report(ctypes.Structure):  # mi32_debug_ws_report
    _fields_ = [("checked", ctypes.c_int), ("damaged", ctypes.c_int), ("zone", ctypes.c_int), ("owner", ctypes.c_int),
                ("part", ctypes.c_int), ("reserved", ctypes.c_int), ("offset", ctypes.c_longlong),
                ("bytes", ctypes.c_size_t), ("name", ctypes.c_char * 16)]


def bind(lib):
    I, Z, VP = ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p
    IP = ctypes.POINTER(I)
    for name, argtypes in (("mi32_debug_ws_guard", [Z]),
                           ("mi32_debug_ws_layout", [VP, I, I, I, ctypes.POINTER(Region), I, IP]),
                           ("mi32_debug_ws_check", [VP, ctypes.POINTER(Report)]),
                           ("mi32_debug_ws_poke", [VP, I, ctypes.c_longlong, ctypes.c_uint]),
                           ("mi32_debug_dense_route", [VP, I, I, I, IP, ctypes.POINTER(Z)])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = I, argtypes
    return lib


@contextlib.contextmanager
def guard(lib, size):
    """The guard mode with zones of ``size`` bytes (rounded up to 256 by the library) inside the block, off behind it."""
    assert lib.mi32_debug_ws_guard(size) == 0
    try:
        yield -(-size // 256) * 256
    finally:
        assert lib.mi32_debug_ws_guard(0) == 0


Entry = namedtuple("Entry", "owner part name offset bytes kind")


def layout(lib, handle, n, batch, elem_bytes):
    """The regions of mi32_debug_ws_layout, in order."""
    count = ctypes.c_int()
    assert lib.mi32_debug_ws_layout(handle, n, batch, elem_bytes, None, 0, ctypes.byref(count)) == 0
    regions = (Region * max(count.value, 1))()
    assert lib.mi32_debug_ws_layout(handle, n, batch, elem_bytes, regions, count.value, ctypes.byref(count)) == 0
    return [Entry(r.owner, r.part, r.name.decode(), r.offset, r.bytes, r.kind) for r in regions[:count.value]]


def carves(entries, owner=None):
    """The entries grouped by carve, in order: ``[((owner, part), [Entry, ...]), ...]``."""
    out = []
    for e in entries:
        if owner is not None and e.owner != owner:
            continue
        if not out or out[-1][0] != (e.owner, e.part):
            out.append(((e.owner, e.part), []))
        out[-1][1].append(e)
    return out


def dense_route(lib, handle, n, batch, elem_bytes):
    out, ws = (ctypes.c_int * 5)(), ctypes.c_size_t()
    assert lib.mi32_debug_dense_route(handle, n, batch, elem_bytes, out, ctypes.byref(ws)) == 0
    return dict(path=out[0], det_steps=out[1], det_first=out[2], np=out[3], bw=out[4], ws=ws.value)


def check(lib, handle):
    r = Report()
    assert lib.mi32_debug_ws_check(handle, ctypes.byref(r)) == 0
    return r


def describe(r):
    return (f"{r.damaged} of {r.checked} zones damaged; first: zone {r.zone} behind region {r.name.decode()!r} "
            f"(owner {r.owner}, part {r.part}), {r.bytes} bytes from offset {r.offset}")


def guard_bytes(row_stride_bytes):
    """max(64 KiB, two rows of the route's padded row stride), rounded up to 256: a stray row cannot jump the zone
    (guard_cases.margin_for's reasoning)."""
    return -(-max(65536, 2 * row_stride_bytes) // 256) * 256


# ---- the cases of tests/test_gpu_workspace_guard.py ---------------------------------------------------------------------
# reference: "steps" / "through" / "mirror64" as guard_cases.INV_ROUTES names the route's oracle (orders up to
# ORACLE_MAX), above that the same call on a second context with the guard off.  knobs: panel_width / block_width of the
# Inverter; env: variables set for the call.
ORACLE_MAX = 1024
Case = namedtuple("Case", "name algo pivoting dtype n batch reference knobs env", defaults=({}, {}))


def _routes(names, batches=None):
    out = []
    for r in guard_cases.INV_ROUTES:
        if r.name not in names:
            continue
        for dt in r.dtypes:
            for n in r.orders:
                for b in batches.get((r.name, n), r.batches) if batches else r.batches:
                    out.append(Case(f"{r.name}-{np.dtype(dt).name}-{n}x{b}", r.algo, r.pivoting, dt, n, b, r.reference))
    return out


# sweep: fp32 at 5 and 257 (batch 3 at 5), fp64 at 5 and 255, no-pivot at 100 in both types
SWEEP_CASES = _routes(("sweep32", "sweep64", "sweep_nopivot"), {("sweep32", 5): (1, 3)})
# blocked fp32: 16, 130, 256, 300, each alone and as a batch of 3
BLOCKED32_CASES = _routes(("blocked32",))
# the seven forced blockings of test_gpu_parity.test_blocked_other_blockings, at that test's orders
OTHER_BLOCKINGS = [(32, 128), (16, 128), (8, 128), (4, 256), (8, 384), (16, 512), (32, 256)]
BLOCKING_CASES = [Case(f"w{w}-bw{bw}-{n}", "blocked", True, F32, n, 1, "through", dict(panel_width=w, block_width=bw))
                  for w, bw in OTHER_BLOCKINGS for n in (200, 640)]
# one order per panel instance: the list of test_gpu_degenerate.test_late_singularity_every_fp32_panel_geometry
PANEL_ORDERS = (200, 500, 1000, 1900, 2048, 3000, 4000)
PANEL_CASES = [Case(f"panel-{n}", "blocked", True, F32, n, 1, "through") for n in PANEL_ORDERS]
N_TALL, N_WIDE = tall_batch_cases.N_TALL, tall_batch_cases.N_WIDE
SCHEDULE_CASES = [
    Case("lookahead-2048", "blocked", True, F32, 2048, 1, "through", {}, {"MI32_LOOKAHEAD_MIN": "2048"}),
    Case("strips-at-end-256x65", "blocked", True, F32, 256, 65, "through"),   # 65 x 4 column tiles > 256
    Case("tall", "blocked", True, F32, N_TALL, 1, "through"),
    Case("tall-pair", "blocked", True, F32, N_TALL, 2, "through"),
    Case("wide", "blocked", True, F32, N_WIDE, 1, "through"),
]
# no-pivot blocked: 520 and 640 in both types; fp64 at both block widths; a batch of 2
NOPIVOT_CASES = _routes(("nopivot_blocked",)) + [
    Case(f"nopivot_blocked-float64-{n}-bw{bw}", "auto", False, F64, n, 1, "through", {}, {"MI32_BLOCK_W64": str(bw)})
    for n in (520, 640) for bw in (64, 128)] + [
    Case(f"nopivot_blocked-{np.dtype(dt).name}-520x2", "auto", False, dt, 520, 2, "through") for dt in (F32, F64)]
# blocked fp64: 256, 300, 700 at the three block widths; 4 x 300
BLOCKED64_CASES = [Case(f"blocked64-{n}-bw{bw}", "auto", True, F64, n, 1, "mirror64", {}, {"MI32_BLOCK_W64": str(bw)})
                   for n in (256, 300, 700) for bw in (64, 128, 256)] + [
    Case("blocked64-300x4", "auto", True, F64, 300, 4, "mirror64")]
INV_CASES = (SWEEP_CASES + BLOCKED32_CASES + BLOCKING_CASES + PANEL_CASES + SCHEDULE_CASES + NOPIVOT_CASES +
             BLOCKED64_CASES)
RESIDUAL_ORDERS, RESIDUAL_BATCH = guard_cases.RESIDUAL_ORDERS, 3
