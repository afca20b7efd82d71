#!/usr/bin/env python3
"""A X = B for mixed orders in one call: what ``Inverter.solve_ragged`` / ``solve_diag_blocks`` cost against the ways a
caller had before.

Shapes, fp32 with partial pivoting:

* the first two of tools/mixed_batch_bench.py -- 16 384 members of orders 3 ... 64 and 4 096 members of orders 65 ... 128,
  the orders capped at 127 (order 128 has no spare column) -- at K = 1 and K = 4 right-hand sides
* the 43 diagonal blocks (orders 1 ... 127) of a 3000 x 3000 matrix at K = 1: applying a block-Jacobi preconditioner

Per shape, in this one process and on the same device-resident data, alternating between the legs call by call (3
warm-up rounds, then the median of 7):

* ``ragged``      -- the one call: ``solve_ragged`` on the packed layout, or ``solve_diag_blocks`` on the matrix
* ``per_order``   -- one ``Inverter.solve`` per distinct order on members already grouped by order (the sort and the
  gather are done once, outside the timed region)
* ``inv_matmul``  -- the diagonal-block shape only: ``inv_diag_blocks`` into a dense zero-filled N x N ``out`` (zeroed once,
  outside the timed region) followed by ``out @ r``

Each call is timed with a host clock between two ``torch.cuda.synchronize()``.  No threshold is asserted: a shape on
which the one call is slower than a leg it replaces is reported as such.

Prints a table and writes ``profiles/vsolve/ragged_solve.json`` (``--out``).  Needs a GPU: there is no fallback.
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

SHAPES = ((16_384, 3, 64), (4_096, 65, 128))   # members, lowest order, highest order (tools/mixed_batch_bench.py)
MAX_ORDER = 127
DIAG_N = 3000


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return None


def make_members(members, lo, hi):
    """(orders, one (count, n, n) batch per distinct order): U(-1, 1) + sqrt(n) I, the orders of mixed_batch_bench.py
    capped at MAX_ORDER."""
    orders = np.minimum(np.random.default_rng(9900 + members % 997 + hi).integers(lo, hi + 1, members), MAX_ORDER)
    rng = np.random.default_rng([9900 + members % 997 + hi, 1])
    by_order = {}
    for n in np.unique(orders):
        count = int((orders == n).sum())
        a = rng.uniform(-1, 1, (count, n, n)) + np.sqrt(n) * np.eye(n)
        by_order[int(n)] = a.astype(np.float32)
    return orders, by_order


def diag_block_orders(total=DIAG_N):
    rng = np.random.default_rng(6)
    orders = []
    while sum(orders) < total:
        orders.append(int(min(rng.integers(1, 129), total - sum(orders))))
    return orders


def timed(torch, legs, warmup, calls):
    ts = {name: [] for name in legs}
    for i in range(warmup + calls):
        for name, fn in legs.items():   # alternating: a drift of the box hits every leg alike
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warmup:
                ts[name].append((time.perf_counter() - t0) * 1e3)
    return {name: {"ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            for name, v in ts.items()}


def compare(row, other):
    row[f"ragged_over_{other}"] = round(row["ragged"]["ms"] / row[other]["ms"], 3)
    row[f"ragged_slower_than_{other}"] = row["ragged"]["ms"] > row[other]["ms"]


def measure_packed(torch, members, lo, hi, k, warmup, calls):
    orders, by_order = make_members(members, lo, hi)
    rng = np.random.default_rng(77 + k)
    # the packed layout, member by member in the caller's order; and the same members grouped by order
    slot = {int(i): (n, j) for n in by_order for j, i in enumerate(np.nonzero(orders == n)[0])}
    b_by_order = {n: rng.uniform(-1, 1, (len(a), n, k)).astype(np.float32) for n, a in by_order.items()}
    flat = np.concatenate([by_order[slot[i][0]][slot[i][1]].reshape(-1) for i in range(members)])
    b = np.concatenate([b_by_order[slot[i][0]][slot[i][1]] for i in range(members)])
    inv = g.Inverter()
    try:
        plan = inv.plan_ragged(orders)
        ta, tb = torch.from_numpy(flat).cuda(), torch.from_numpy(b).cuda()
        x = torch.empty_like(tb)
        st = torch.empty(members, dtype=torch.int32, device="cuda")
        groups = [(torch.from_numpy(a).cuda(), torch.from_numpy(b_by_order[n]).cuda()) for n, a in by_order.items()]
        groups = [(a, bb, torch.empty_like(bb), torch.empty(len(a), dtype=torch.int32, device="cuda")) for a, bb in groups]

        def per_order():
            for a, bb, xx, ss in groups:
                inv.solve(a, bb, out=xx, status=ss)

        row = {"shape": "packed", "members": members, "orders": [int(orders.min()), int(orders.max())],
               "distinct_orders": len(by_order), "nrhs": k, "dtype": "float32", "pivoting": True,
               "ragged_launches": len(inv.resolved_solve_ragged(orders, k)),
               "per_order_launches": sum(inv.resolved_solve(n, k)[1] for n in by_order)}
        row.update(timed(torch, {"ragged": lambda: inv.solve_ragged(plan, ta, tb, out=x, status=st),
                                 "per_order": per_order}, warmup, calls))
        compare(row, "per_order")
        # the two legs computed the same thing
        off = np.concatenate(([0], np.cumsum(orders)))
        xh = x.cpu().numpy()
        xs = {n: grp[2].cpu().numpy() for n, grp in zip(by_order, groups)}
        same = all(np.array_equal(xs[slot[i][0]][slot[i][1]], xh[off[i]:off[i + 1]]) for i in range(0, members, 97))
        row["legs_bit_identical_on_sampled_members"] = bool(same)
        row["nonzero_status"] = int((st != 0).sum())
        plan.close()
    finally:
        inv.close()
    return row


def measure_diag(torch, k, warmup, calls):
    orders = diag_block_orders()
    rng = np.random.default_rng(78)
    m = np.zeros((DIAG_N, DIAG_N), np.float32)
    at = 0
    for n in orders:
        m[at:at + n, at:at + n] = rng.uniform(-1, 1, (n, n)) + np.sqrt(n) * np.eye(n)
        at += n
    r = rng.uniform(-1, 1, (DIAG_N,) if k == 1 else (DIAG_N, k)).astype(np.float32)
    inv = g.Inverter()
    try:
        tm, tr = torch.from_numpy(m).cuda(), torch.from_numpy(r).cuda()
        z = torch.empty_like(tr)
        dense = torch.zeros_like(tm)
        z2 = torch.empty_like(tr)

        def inv_matmul():
            inv.inv_diag_blocks(tm, orders, out=dense)
            return torch.matmul(dense, tr, out=z2)

        row = {"shape": "diagonal blocks", "matrix_order": DIAG_N, "members": len(orders),
               "orders": [min(orders), max(orders)], "nrhs": k, "dtype": "float32", "pivoting": True,
               "ragged_launches": len(inv.resolved_solve_ragged(orders, k))}
        row.update(timed(torch, {"ragged": lambda: inv.solve_diag_blocks(tm, orders, tr, out=z),
                                 "inv_matmul": inv_matmul}, warmup, calls))
        compare(row, "inv_matmul")
        _, st = inv.solve_diag_blocks(tm, orders, tr, out=z)
        torch.cuda.synchronize()
        row["nonzero_status"] = int((st != 0).sum())
        row["max_abs_difference_of_the_legs"] = float((z - z2).abs().max())
    finally:
        inv.close()
    return row


def show(row):
    other = "per_order" if "per_order" in row else "inv_matmul"
    print(f"{row['shape']:15s} members={row['members']:6d} orders {row['orders'][0]:3d}...{row['orders'][1]:3d} "
          f"K={row['nrhs']} one call {row['ragged']['ms']:8.3f} ms ({row['ragged_launches']} launches) | {other} "
          f"{row[other]['ms']:8.3f} ms (one call x{row['ragged_over_' + other]:.3f}"
          f"{', SLOWER' if row['ragged_slower_than_' + other] else ''})", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vsolve", "ragged_solve.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--commit", default=None, help="what to record as the commit measured (default: git HEAD)")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("ragged_solve_bench.py needs a GPU; there is no fallback")
    torch.cuda.set_device(0)
    rows = []
    for members, lo, hi in SHAPES:
        for k in (1, 4):
            rows.append(measure_packed(torch, members, lo, hi, k, args.warmup, args.calls))
            show(rows[-1])
    rows.append(measure_diag(torch, 1, args.warmup, args.calls))
    show(rows[-1])
    doc = {"device": torch.cuda.get_device_name(0), "commit": args.commit or commit(),
           "library_version": _lib.load().mi32_version(),
           "method": f"median of {args.calls} calls after {args.warmup} warm-ups, the legs alternating call by call, "
                     "torch.cuda.synchronize() around each call, device-resident tensors, one process",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
