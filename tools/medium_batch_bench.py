#!/usr/bin/env python3
"""Large batches of matrices of order 65 ... 128: the workgroup-resident path against the path AUTO resolves to today.

For n in {65, 80, 96, 112, 128} x B in {256, 2048, 16384} (and the workgroup path alone at (65, 70 000), more members
than a grid y / z dimension holds) both paths invert the same device-resident fp32 batch with partial pivoting, in
this one process, one after the other: 3 warm-up calls, then the median of 7 calls, each between two
``torch.cuda.synchronize()`` -- the timing protocol of tools/small_batch_bench.py.  The blocked and sweep paths are
not touched by the workgroup path, so timing them here is timing what the library did before it.  Per shape and
path: ms per call, matrices per second, effective GB/s (one read and one write of every element, 8 n^2 B bytes, over
the time; the HBM spec is 8000 GB/s) and ``mi32_workspace_bytes``.  A shape whose AUTO workspace exceeds half of the
free device memory is reported as not run.  Extra legs, workgroup against AUTO as well: fp64 and fp32 without
pivoting at (96, 2048) and (128, 1024).

Prints a table and writes ``profiles/workgroup/medium_batch.json`` (``--out``).  Needs a GPU: there is no fallback.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gpu_matrix_inversion_amd as g  # noqa: E402
from gpu_matrix_inversion_amd import _lib  # noqa: E402

ORDERS = (65, 80, 96, 112, 128)
BATCHES = (256, 2_048, 16_384)
ABOVE_GRID_LIMIT = (65, 70_000)
EXTRA_SHAPES = ((96, 2_048), (128, 1_024))
HBM_SPEC_GBS = 8000.0
ALGO_LABEL = {_lib.ALGO_SWEEP: "sweep", _lib.ALGO_BLOCKED: "blocked", _lib.ALGO_RESIDENT: "resident",
              _lib.ALGO_WORKGROUP: "workgroup"}


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return None


def make_batch(torch, n, batch, dtype, dominant):
    rng = np.random.default_rng(1000 * n + batch % 997)
    a = rng.uniform(-1, 1, (batch, n, n)).astype(np.float32)
    if dominant:   # the no-pivot variant's inputs
        a[:, np.arange(n), np.arange(n)] = np.abs(a).sum(axis=2) + 1.0
    else:
        a += np.float32(np.sqrt(n)) * np.eye(n, dtype=np.float32)
    return torch.from_numpy(a.astype(dtype)).cuda()


def timed(torch, inv, a, warmup, calls):
    out = torch.empty_like(a)
    st = torch.empty(a.shape[0], dtype=torch.int32, device=a.device)
    ts = []
    for i in range(warmup + calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        inv.inv(a, out=out, status=st)
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    bad = int((st != 0).sum())
    return statistics.median(ts), (min(ts), max(ts)), out, bad


def leg(ms, n, batch, elem_bytes):
    return {"ms": round(ms, 4), "matrices_per_s": round(batch / (ms * 1e-3)),
            "effective_GBps": round(2 * elem_bytes * n * n * batch / (ms * 1e-3) / 1e9, 1)}


def rows_per_thread(n, elem_bytes):
    threads, rows, top = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().mi32_resolve_workgroup(None, n, elem_bytes, ctypes.byref(threads), ctypes.byref(rows),
                                                  ctypes.byref(top)), "mi32_resolve_workgroup")
    return rows.value


def measure(torch, n, batch, dtype, pivoting, with_parent, warmup, calls):
    lib = _lib.load()
    elem = np.dtype(dtype).itemsize
    a = make_batch(torch, n, batch, dtype, dominant=not pivoting)
    row = {"n": n, "batch": batch, "dtype": np.dtype(dtype).name, "pivoting": pivoting,
           "bytes_moved": 2 * elem * n * n * batch}
    wg = g.Inverter(algo="workgroup", pivoting=pivoting)
    try:
        assert wg.resolved_algo(n, batch) == _lib.ALGO_WORKGROUP
        ms, best, x_wg, bad = timed(torch, wg, a, warmup, calls)
    finally:
        wg.close()
    row["workgroup"] = dict(leg(ms, n, batch, elem), min_ms=round(best[0], 4), max_ms=round(best[1], 4),
                            nonzero_status=bad,
                            workspace_bytes=int(lib.mi32_workspace_bytes(n, batch, _lib.ALGO_WORKGROUP)),
                            rows_per_thread=rows_per_thread(n, elem))
    if not with_parent:
        row["parent"] = "not run: the other paths cannot launch more than 65535 members"
        return row
    auto = g.Inverter(algo="auto", pivoting=pivoting)
    try:
        algo = auto.resolved_algo(n, batch) if elem == 4 else (
            _lib.ALGO_BLOCKED if auto.resolved_blocking_f64(n) else _lib.ALGO_SWEEP)
        ws = int(lib.mi32_workspace_bytes(n, batch, _lib.ALGO_AUTO)) if elem == 4 else None
        free, _ = torch.cuda.mem_get_info()
        if ws is not None and ws > free // 2:
            row["parent"] = f"not run, workspace {ws / 2**30:.1f} GiB"
            row["parent_workspace_bytes"] = ws
            return row
        if elem == 4:
            auto.reserve(n, batch)
        ms_p, best_p, x_par, bad_p = timed(torch, auto, a, warmup, calls)
    finally:
        auto.close()
    row["parent"] = dict(leg(ms_p, n, batch, elem), min_ms=round(best_p[0], 4), max_ms=round(best_p[1], 4),
                         nonzero_status=bad_p,
                         algo=ALGO_LABEL[algo], workspace_bytes=ws)
    row["speedup"] = round(ms_p / ms, 2)
    row["same_values"] = bool(torch.equal(x_wg, x_par))
    return row


def show(row):
    r = row["workgroup"]
    head = f"{row['dtype']:8s} piv={int(row['pivoting'])} n={row['n']:3d} B={row['batch']:8d}  workgroup {r['ms']:9.3f} ms " \
           f"{r['matrices_per_s']:12d} mat/s {r['effective_GBps']:7.1f} GB/s ({100 * r['effective_GBps'] / HBM_SPEC_GBS:4.1f}% of spec)"
    p = row["parent"]
    if isinstance(p, dict):
        head += f" | {p['algo']:7s} {p['ms']:10.3f} ms  x{row['speedup']:.2f}  same values: {row['same_values']}"
    else:
        head += f" | parent: {p}"
    print(head, flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "workgroup", "medium_batch.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--commit", default=None, help="what to record as the commit measured (default: git HEAD)")
    ap.add_argument("--quick", action="store_true", help="only the two shapes the timing test asserts, and (128, 2048)")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("medium_batch_bench.py needs a GPU; there is no fallback")
    torch.cuda.set_device(0)
    rows = []
    not_measured = []
    shapes = [(65, 4_096), (96, 2_048), (128, 2_048)] if args.quick else [(n, b) for n in ORDERS for b in BATCHES]
    for n, b in shapes:
        rows.append(measure(torch, n, b, np.float32, True, True, args.warmup, args.calls))
        show(rows[-1])
    if not args.quick:
        rows.append(measure(torch, *ABOVE_GRID_LIMIT, np.float32, True, False, args.warmup, args.calls))
        show(rows[-1])
        for n, b in EXTRA_SHAPES:
            for dtype, piv in ((np.float64, True), (np.float32, False), (np.float64, False)):
                rows.append(measure(torch, n, b, dtype, piv, True, args.warmup, args.calls))
                show(rows[-1])
    else:
        not_measured = ["every shape of the full grid but the three above", "the shape above the grid limit",
                        "the fp64 and no-pivot legs"]
    doc = {"device": torch.cuda.get_device_name(0), "commit": args.commit or commit(), "library_version": _lib.load().mi32_version(),
           "method": f"median of {args.calls} calls after {args.warmup} warm-ups, torch.cuda.synchronize() around each call, "
                     "device-resident tensors, both paths in one process, AUTO's workspace reserved first",
           "hbm_spec_GBps": HBM_SPEC_GBS, "not_measured": not_measured, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
