#!/usr/bin/env python3
"""Large batches of fp32 matrices of order 129 ... 256: the wide workgroup-resident path against the path AUTO resolves
to today.

For (n, B) in {(129, 4096), (160, 2048), (192, 2048), (224, 1024), (256, 1024), (256, 100 000)} both paths invert the
same device-resident fp32 batch with partial pivoting, in this one process, one after the other: 3 warm-up calls, then
the median of 7 calls, each between two ``torch.cuda.synchronize()`` -- the timing protocol of
tools/medium_batch_bench.py.  The blocked path is not touched by the wide path, so timing it here is timing what the
library did before it.  Per shape and path: ms per call, matrices per second, effective GB/s (one read and one write of
every element, 8 n^2 B bytes, over the time; the HBM spec is 8000 GB/s) and ``mi32_workspace_bytes``.  AUTO is reported
as not run where it cannot be launched (more than 65535 members: the batch index is a grid y / z coordinate) or where
its workspace exceeds half of the free device memory.  A batch holds at most 1024 distinct matrices, repeated in order.

Not measured here: the no-pivot variant and the determinant twin.

Prints a table and writes ``profiles/wide/wide_batch.json`` (``--out``).  Needs a GPU: there is no fallback.
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

SHAPES = ((129, 4_096), (160, 2_048), (192, 2_048), (224, 1_024), (256, 1_024), (256, 100_000))
QUICK_SHAPES = ((160, 2_048), (256, 1_024))
GRID_LIMIT = 65_535
DISTINCT = 1_024
HBM_SPEC_GBS = 8000.0
ALGO_LABEL = {_lib.ALGO_SWEEP: "sweep", _lib.ALGO_BLOCKED: "blocked", _lib.ALGO_RESIDENT: "resident",
              _lib.ALGO_WORKGROUP: "workgroup", _lib.ALGO_WIDE: "wide"}


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return None


def make_batch(torch, n, batch):
    k = min(batch, DISTINCT)
    rng = np.random.default_rng(1000 * n + batch % 997)
    a = rng.uniform(-1, 1, (k, n, n)).astype(np.float32)
    a += np.float32(np.sqrt(n)) * np.eye(n, dtype=np.float32)
    t = torch.from_numpy(a).cuda()
    if k == batch:
        return t
    return t[torch.arange(batch, device=t.device) % k].contiguous()


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


def leg(ms, n, batch):
    return {"ms": round(ms, 4), "matrices_per_s": round(batch / (ms * 1e-3)),
            "effective_GBps": round(8 * n * n * batch / (ms * 1e-3) / 1e9, 1)}


def wide_class(n):
    threads, rows, top = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().mi32_resolve_wide(None, n, 4, ctypes.byref(threads), ctypes.byref(rows), ctypes.byref(top)),
               "mi32_resolve_wide")
    return threads.value, rows.value


def measure(torch, n, batch, warmup, calls):
    lib = _lib.load()
    a = make_batch(torch, n, batch)
    row = {"n": n, "batch": batch, "dtype": "float32", "pivoting": True, "bytes_moved": 8 * n * n * batch}
    wide = g.Inverter(algo="wide")
    try:
        assert wide.resolved_algo(n, batch) == _lib.ALGO_WIDE
        ms, best, x_wide, bad = timed(torch, wide, a, warmup, calls)
    finally:
        wide.close()
    threads, rows = wide_class(n)
    row["wide"] = dict(leg(ms, n, batch), min_ms=round(best[0], 4), max_ms=round(best[1], 4), nonzero_status=bad,
                       workspace_bytes=int(lib.mi32_workspace_bytes(n, batch, _lib.ALGO_WIDE)), threads=threads,
                       rows_per_thread=rows)
    ws = int(lib.mi32_workspace_bytes(n, batch, _lib.ALGO_AUTO))
    row["parent_workspace_bytes"] = ws
    auto = g.Inverter(algo="auto")
    try:
        algo = auto.resolved_algo(n, batch)
        row["parent_algo"] = ALGO_LABEL[algo]
        free, _ = torch.cuda.mem_get_info()
        if batch > GRID_LIMIT:
            row["parent"] = f"cannot be launched: more than {GRID_LIMIT} members (workspace {ws / 2**30:.1f} GiB)"
            return row
        if ws > free // 2:
            row["parent"] = f"not run, workspace {ws / 2**30:.1f} GiB"
            return row
        auto.reserve(n, batch)
        ms_p, best_p, x_par, bad_p = timed(torch, auto, a, warmup, calls)
    finally:
        auto.close()
    row["parent"] = dict(leg(ms_p, n, batch), min_ms=round(best_p[0], 4), max_ms=round(best_p[1], 4),
                         nonzero_status=bad_p, algo=ALGO_LABEL[algo],
                         workspace_bytes=ws)
    row["speedup"] = round(ms_p / ms, 2)
    row["same_values"] = bool(torch.equal(x_wide, x_par))
    return row


def show(row):
    r = row["wide"]
    head = f"n={row['n']:3d} B={row['batch']:7d}  wide {r['ms']:9.3f} ms {r['matrices_per_s']:10d} mat/s " \
           f"{r['effective_GBps']:7.1f} GB/s ({100 * r['effective_GBps'] / HBM_SPEC_GBS:4.1f}% of spec)"
    p = row["parent"]
    if isinstance(p, dict):
        head += f" | {p['algo']:7s} {p['ms']:10.3f} ms  ws {p['workspace_bytes'] / 2**20:8.1f} MiB  x{row['speedup']:.2f}  " \
                f"same values: {row['same_values']}"
    else:
        head += f" | parent: {p}"
    print(head, flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide", "wide_batch.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--commit", default=None, help="what to record as the commit measured (default: git HEAD)")
    ap.add_argument("--quick", action="store_true", help="only the two shapes the timing test asserts")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("wide_batch_bench.py needs a GPU; there is no fallback")
    torch.cuda.set_device(0)
    rows = []
    for n, b in (QUICK_SHAPES if args.quick else SHAPES):
        rows.append(measure(torch, n, b, args.warmup, args.calls))
        show(rows[-1])
    not_measured = ["the no-pivot variant", "the determinant twin (gj_wide_det_kernel)"]
    if args.quick:
        not_measured.append("every shape but the two the timing test asserts")
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
