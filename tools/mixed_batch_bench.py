#!/usr/bin/env python3
"""Batches of mixed orders: one variable-size call against one uniform call per distinct order.

For 16 384 members with orders uniform in 3 ... 64, 4 096 members in 65 ... 128 and 65 536 members in 1 ... 128, the
same device-resident members are inverted two ways in this one process, alternating call by call: one
``Inverter.inv_ragged`` call on the packed batch (one status memset, at most eight launches), and the best a user
could do without it -- the members ALREADY grouped by order into contiguous uniform device batches and one
``Inverter(algo="workgroup").inv`` call per distinct order (the host-side sort and gather is left out of the baseline,
which favours the baseline).  3 warm-up rounds, then the median of 7 calls of each side, each call between two
``torch.cuda.synchronize()`` -- the timing protocol of tools/small_batch_bench.py.  fp32 with pivoting for every shape;
fp64 and fp32 without pivoting for the first two.  Every member of the two results is compared bit for bit.

Prints a table and writes ``profiles/vbatch/mixed_batch.json`` (``--out``); a shape that was not run (``--quick``:
only the two shapes the timing test asserts) is recorded as not measured.  Needs a GPU: there is no fallback.
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

SHAPES = ((16_384, 3, 64), (4_096, 65, 128), (65_536, 1, 128))   # members, lowest order, highest order
EXTRA_LEGS = ((np.float64, True), (np.float32, False))           # on the first two shapes
HBM_SPEC_GBS = 8000.0


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return None


def make_members(members, lo, hi, dtype, dominant):
    """(orders, {order: (indices, batch (k, n, n))}): U(-1, 1) + sqrt(n) I, or strictly diagonally dominant rows for
    the no-pivot variant."""
    rng = np.random.default_rng(9900 + members % 997 + hi)
    orders = rng.integers(lo, hi + 1, members)
    groups = {}
    for n in np.unique(orders):
        idx = np.nonzero(orders == n)[0]
        a = rng.uniform(-1, 1, (idx.size, n, n))
        if dominant:
            a[:, np.arange(n), np.arange(n)] = np.abs(a).sum(axis=2) + 1.0
        else:
            a += np.sqrt(n) * np.eye(n)
        groups[int(n)] = (idx, a.astype(dtype))
    return orders, groups


def timed_pair(torch, one, loop, warmup, calls):
    t_one, t_loop = [], []
    for i in range(warmup + calls):
        for fn, ts in ((one, t_one), (loop, t_loop)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
    return t_one, t_loop


def leg(ts, members, bytes_moved):
    ms = statistics.median(ts)
    return {"ms": round(ms, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
            "members_per_s": round(members / (ms * 1e-3)),
            "effective_GBps": round(bytes_moved / (ms * 1e-3) / 1e9, 1)}


def measure(torch, members, lo, hi, dtype, pivoting, warmup, calls):
    orders, groups = make_members(members, lo, hi, dtype, dominant=not pivoting)
    elem = np.dtype(dtype).itemsize
    sq = orders.astype(np.int64) ** 2
    off = np.concatenate(([0], np.cumsum(sq)))
    flat = np.empty(int(off[-1]), dtype)
    for n, (idx, a) in groups.items():
        for k, b in enumerate(idx):
            flat[off[b]:off[b + 1]] = a[k].reshape(-1)
    row = {"members": members, "orders": [lo, hi], "distinct_orders": len(groups), "dtype": np.dtype(dtype).name,
           "pivoting": pivoting, "bytes_moved": int(2 * elem * off[-1])}
    inv = g.Inverter(algo="workgroup", pivoting=pivoting)
    plan = inv.plan_ragged(orders)
    try:
        row["class_counts"] = list(plan.class_counts)
        row["launches_one_call"] = sum(1 for c in plan.class_counts if c)
        a_flat = torch.from_numpy(flat).cuda()
        out_flat = torch.empty_like(a_flat)
        st_flat = torch.empty(members, dtype=torch.int32, device="cuda")
        dev = {n: torch.from_numpy(a).cuda() for n, (_, a) in groups.items()}
        outs = {n: torch.empty_like(t) for n, t in dev.items()}
        sts = {n: torch.empty(t.shape[0], dtype=torch.int32, device="cuda") for n, t in dev.items()}

        def one():
            inv.inv_ragged(plan, a_flat, out=out_flat, status=st_flat)

        def loop():
            for n in dev:
                inv.inv(dev[n], out=outs[n], status=sts[n])

        t_one, t_loop = timed_pair(torch, one, loop, warmup, calls)
        got = out_flat.cpu().numpy()
        same = True
        for n, (idx, _) in groups.items():
            ref = outs[n].cpu().numpy()
            same = same and all(np.array_equal(got[off[b]:off[b + 1]], ref[k].reshape(-1)) for k, b in enumerate(idx))
        bad = int((st_flat != 0).sum()) + sum(int((s != 0).sum()) for s in sts.values())
    finally:
        plan.close()
        inv.close()
    row["one_call"] = leg(t_one, members, row["bytes_moved"])
    row["call_per_order"] = leg(t_loop, members, row["bytes_moved"])
    row["speedup"] = round(row["call_per_order"]["ms"] / row["one_call"]["ms"], 2)
    row["same_values"] = bool(same)
    row["nonzero_status"] = bad
    return row


def show(row):
    o, p = row["one_call"], row["call_per_order"]
    print(f"{row['dtype']:8s} piv={int(row['pivoting'])} {row['members']:6d} members, orders {row['orders'][0]:3d}..{row['orders'][1]:3d}: "
          f"one call ({row['launches_one_call']} launches) {o['ms']:9.3f} ms {o['effective_GBps']:7.1f} GB/s | "
          f"{row['distinct_orders']:3d} calls {p['ms']:9.3f} ms  x{row['speedup']:.2f}  same values: {row['same_values']}",
          flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vbatch", "mixed_batch.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--commit", default=None, help="what to record as the commit measured (default: git HEAD)")
    ap.add_argument("--quick", action="store_true", help="only the two shapes the timing test asserts, fp32 with pivoting")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("mixed_batch_bench.py needs a GPU; there is no fallback")
    torch.cuda.set_device(0)
    legs = [(s, np.float32, True) for s in (SHAPES[:2] if args.quick else SHAPES)]
    skipped = [(s, np.float32, True) for s in SHAPES[2:]] if args.quick else []
    for dtype, piv in EXTRA_LEGS:
        (skipped if args.quick else legs).extend((s, dtype, piv) for s in SHAPES[:2])
    rows = []
    for (members, lo, hi), dtype, piv in legs:
        rows.append(measure(torch, members, lo, hi, dtype, piv, args.warmup, args.calls))
        show(rows[-1])
    not_measured = [f"{m} members, orders {lo}..{hi}, {np.dtype(d).name}, pivoting {'on' if p else 'off'}"
                    for (m, lo, hi), d, p in skipped]
    doc = {"device": torch.cuda.get_device_name(0), "commit": args.commit or commit(),
           "library_version": _lib.load().mi32_version(),
           "method": f"median of {args.calls} calls after {args.warmup} warm-ups, torch.cuda.synchronize() around each call, "
                     "device-resident tensors, both sides in one process alternating call by call; baseline: members "
                     "already grouped by order, one Inverter(algo='workgroup').inv call per distinct order",
           "hbm_spec_GBps": HBM_SPEC_GBS, "not_measured": not_measured, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
