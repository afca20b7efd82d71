#!/usr/bin/env python3
"""Diagnostic (not part of the product): A X = B at widths of 33 ... 64, the shapes that reach the 64-lane instances of
gj_resident_solve_kernel / gj_resident_solve_vkernel, which no other tool times.

    python tools/solve64_bench.py --out profiles/resident_body/solve64.json [--commit LABEL]

* uniform fp64 solve with pivoting, order 48, one column, 2048 members
* variable-size solve, fp32 and fp64, with and without pivoting: 4096 members of orders 33 ... 60, four columns
Median of 7 calls after 3 warm-ups, each call between two torch.cuda.synchronize(), fastest and slowest call recorded:
the protocol of tools/solve_bench.py.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gpu_matrix_inversion_amd as g  # noqa: E402


def timed(fn, warmup=3, calls=7):
    ts = []
    for i in range(warmup + calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return {"ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def dominant(rng, count, n, dtype):
    a = rng.uniform(-1, 1, (count, n, n))
    a[:, np.arange(n), np.arange(n)] = np.abs(a).sum(axis=2) + 1.0
    return a.astype(dtype)


def uniform_leg(n, k, batch, dtype, pivoting):
    rng = np.random.default_rng(5000 + n)
    a = dominant(rng, batch, n, dtype)
    b = rng.uniform(-1, 1, (batch, n, k)).astype(dtype)
    inv = g.Inverter(pivoting=pivoting)
    try:
        ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        x = torch.empty_like(tb)
        st = torch.empty(batch, dtype=torch.int32, device="cuda")
        row = {"shape": f"uniform solve {np.dtype(dtype).name} piv={int(pivoting)} n={n} K={k} B={batch}",
               "lanes": inv.resolved_solve(n, k, np.dtype(dtype).itemsize)[2]}
        row.update(timed(lambda: inv.solve(ta, tb, out=x, status=st)))
        row["nonzero_status"] = int((st != 0).sum())
    finally:
        inv.close()
    return row


def ragged_leg(members, lo, hi, k, dtype, pivoting):
    rng = np.random.default_rng(6000 + hi)
    orders = rng.integers(lo, hi + 1, members)
    flat = np.concatenate([dominant(rng, 1, int(n), dtype).reshape(-1) for n in orders])
    b = rng.uniform(-1, 1, (int(orders.sum()), k)).astype(dtype)
    inv = g.Inverter(pivoting=pivoting)
    try:
        plan = inv.plan_ragged(orders)
        ta, tb = torch.from_numpy(flat).cuda(), torch.from_numpy(b).cuda()
        x = torch.empty_like(tb)
        st = torch.empty(members, dtype=torch.int32, device="cuda")
        launches = inv.resolved_solve_ragged(orders, k)
        row = {"shape": f"ragged solve {np.dtype(dtype).name} piv={int(pivoting)} {members} members {lo}..{hi} K={k}",
               "launches": [list(l) for l in launches]}
        row.update(timed(lambda: inv.solve_ragged(plan, ta, tb, out=x, status=st)))
        row["nonzero_status"] = int((st != 0).sum())
        plan.close()
    finally:
        inv.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rows = [uniform_leg(48, 1, 2048, np.float64, True)]
    for dtype in (np.float32, np.float64):
        for piv in (False, True):
            rows.append(ragged_leg(4096, 33, 60, 4, dtype, piv))
    for r in rows:
        print(f"{r['shape']:62s} {r['ms']:8.3f} ms ({r['min_ms']:.3f} ... {r['max_ms']:.3f}) status!=0: {r['nonzero_status']}",
              flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "commit": args.commit,
           "method": "median of 7 calls after 3 warm-ups, torch.cuda.synchronize() around each call, device-resident "
                     "tensors, strictly diagonally dominant members; Inverter.solve / Inverter.solve_ragged",
           "rows": rows}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
