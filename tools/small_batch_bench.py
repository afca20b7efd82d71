#!/usr/bin/env python3
"""Large batches of small matrices: the register-resident path against the path AUTO resolves to today.

For n in {4, 8, 16, 32, 64} x B in {1000, 16384, 65535} (and the resident path alone at (8, 1 000 000)) both paths
invert the same device-resident fp32 batch with partial pivoting, in this one process, one after the other:
3 warm-up calls, then the median of 7 calls, each between two ``torch.cuda.synchronize()``.  Neither the sweep
nor the blocked path is touched by the resident path, so timing them here is timing what the library did
before it.  Per shape and path: ms per call, matrices per second, effective GB/s (one read and one write of
every element, 8 n^2 B bytes, over the time; the HBM spec is 8000 GB/s) and ``mi32_workspace_bytes``.  A shape
whose AUTO workspace exceeds half of the free device memory is reported as not run.  Extra legs, resident against
AUTO as well: fp64 at (32, 4096) and (64, 2048), fp32 without pivoting at (32, 4096).

Prints a table and writes ``profiles/resident/small_batch.json`` (``--out``).  Needs a GPU: there is no fallback.
"""
import argparse
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

ORDERS = (4, 8, 16, 32, 64)
BATCHES = (1_000, 16_384, 65_535)
HBM_SPEC_GBS = 8000.0
ALGO_LABEL = {_lib.ALGO_SWEEP: "sweep", _lib.ALGO_BLOCKED: "blocked", _lib.ALGO_RESIDENT: "resident"}


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


def measure(torch, n, batch, dtype, pivoting, with_parent, warmup, calls):
    lib = _lib.load()
    elem = np.dtype(dtype).itemsize
    a = make_batch(torch, n, batch, dtype, dominant=not pivoting)
    row = {"n": n, "batch": batch, "dtype": np.dtype(dtype).name, "pivoting": pivoting,
           "bytes_moved": 2 * elem * n * n * batch}
    res = g.Inverter(algo="resident", pivoting=pivoting)
    try:
        assert res.resolved_algo(n, batch) == _lib.ALGO_RESIDENT
        ms, best, x_res, bad = timed(torch, res, a, warmup, calls)
    finally:
        res.close()
    row["resident"] = dict(leg(ms, n, batch, elem), min_ms=round(best[0], 4), max_ms=round(best[1], 4),
                           nonzero_status=bad,
                           workspace_bytes=int(lib.mi32_workspace_bytes(n, batch, _lib.ALGO_RESIDENT)),
                           lanes_per_matrix=int(g_lanes(n, elem)))
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
        ms_p, best_p, x_par, bad_p = timed(torch, auto, a, warmup, calls)
    finally:
        auto.close()
    row["parent"] = dict(leg(ms_p, n, batch, elem), min_ms=round(best_p[0], 4), max_ms=round(best_p[1], 4),
                         nonzero_status=bad_p,
                         algo=ALGO_LABEL[algo], workspace_bytes=ws)
    row["speedup"] = round(ms_p / ms, 2)
    row["same_values"] = bool(torch.equal(x_res, x_par))
    return row


def g_lanes(n, elem_bytes):
    import ctypes

    lanes, top = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().mi32_resolve_resident(None, n, elem_bytes, ctypes.byref(lanes), ctypes.byref(top)),
               "mi32_resolve_resident")
    return lanes.value


def show(row):
    r = row["resident"]
    head = f"{row['dtype']:8s} piv={int(row['pivoting'])} n={row['n']:3d} B={row['batch']:8d}  resident {r['ms']:9.3f} ms " \
           f"{r['matrices_per_s']:12d} mat/s {r['effective_GBps']:7.1f} GB/s ({100 * r['effective_GBps'] / HBM_SPEC_GBS:4.1f}% of spec)"
    p = row["parent"]
    if isinstance(p, dict):
        head += f" | {p['algo']:7s} {p['ms']:10.3f} ms  x{row['speedup']:.1f}  same values: {row['same_values']}"
    else:
        head += f" | parent: {p}"
    print(head, flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resident", "small_batch.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--commit", default=None, help="what to record as the commit measured (default: git HEAD)")
    ap.add_argument("--quick", action="store_true", help="only the three shapes the timing test asserts")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("small_batch_bench.py needs a GPU; there is no fallback")
    torch.cuda.set_device(0)
    rows = []
    shapes = [(8, 16_384), (32, 4_096), (64, 2_048)] if args.quick else [(n, b) for n in ORDERS for b in BATCHES]
    for n, b in shapes:
        rows.append(measure(torch, n, b, np.float32, True, True, args.warmup, args.calls))
        show(rows[-1])
    if not args.quick:
        rows.append(measure(torch, 8, 1_000_000, np.float32, True, False, args.warmup, args.calls))
        show(rows[-1])
        for n, b, dtype, piv in ((32, 4_096, np.float64, True), (64, 2_048, np.float64, True), (32, 4_096, np.float32, False)):
            rows.append(measure(torch, n, b, dtype, piv, True, args.warmup, args.calls))
            show(rows[-1])
    doc = {"device": torch.cuda.get_device_name(0), "commit": args.commit or commit(), "library_version": _lib.load().mi32_version(),
           "method": f"median of {args.calls} calls after {args.warmup} warm-ups, torch.cuda.synchronize() around each call, "
                     "device-resident tensors, both paths in one process",
           "hbm_spec_GBps": HBM_SPEC_GBS, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
