#!/usr/bin/env python3
"""z = blockdiag(X) r on stored inverses of mixed orders in one call: what ``Inverter.apply_ragged`` /
``apply_diag_blocks`` cost against the ways a caller had before.

Shapes, fp32 (those of tools/ragged_solve_bench.py, orders capped at 127 so that the solve leg takes them):

* 16 384 members of orders 3 ... 64 and 4 096 members of orders 65 ... 127, at K = 1 and K = 4 right-hand sides
* the 43 diagonal blocks (orders 1 ... 127) of a 3000 x 3000 matrix at K = 1: applying a block-Jacobi preconditioner

Per shape, in this one process and on the same device-resident data, alternating between the legs call by call (3
warm-up rounds, then the median of 7, min ... max recorded):

* ``apply``       -- the one call on the stored inverses: ``apply_ragged`` on the packed layout, or
  ``apply_diag_blocks`` on the packed inverses of ``inv_diag_blocks(packed=True)``
  (the member addresses of r and z come from ``RaggedPlan.row_pointers``, cached after the first call, as those of
  the solve leg below do)
* ``solve``       -- ``solve_ragged`` / ``solve_diag_blocks`` on the matrices themselves, per application: the way until now
* ``bmm``         -- one ``torch.bmm`` per distinct order on inverses already grouped by order (the sort and the gather
  are done once, outside the timed region)
* ``dense``       -- the diagonal-block shape only: ``out @ r`` with the dense N x N inverse of ``inv_diag_blocks``

For every ``apply`` row the bytes of X + R + Z over the time are reported as GB/s, beside the 8 TB/s HBM specification
and the 6.29 TB/s a device-to-device copy reaches on this part, and whether X fits the 256 MB Infinity Cache: the calls
re-read the same inverses, as a Krylov loop does, so an X that fits is served from that cache and the figure is no HBM
rate.  Beside the call's wall time the time of its kernels alone is reported (the context's event timing around each
launch, median of 7 calls), since a call of a few launches on tens of megabytes is partly the host's.  Each call is
timed with a host clock between two ``torch.cuda.synchronize()``.  No threshold is asserted: a
shape on which the one call is slower than a leg it replaces is reported as such.

Prints a table and writes ``profiles/apply/ragged_apply.json`` (``--out``).  Needs a GPU: there is no fallback.
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

SHAPES = ((16_384, 3, 64), (4_096, 65, 128))   # members, lowest order, highest order (tools/ragged_solve_bench.py)
MAX_ORDER = 127
DIAG_N = 3000
HBM_SPEC_TBS = 8.0
COPY_TBS = 6.29
INFINITY_CACHE_BYTES = 256 * 2 ** 20


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return None


def make_members(members, lo, hi):
    """(orders, one (count, n, n) batch per distinct order): U(-1, 1) + sqrt(n) I, the orders of
    tools/ragged_solve_bench.py."""
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


def kernel_ms(torch, inv, fn, calls):
    """Median over `calls` calls of the time between the events that bracket the call's launches (the context's
    per-class timing): what the kernels take without the host's share of the call."""
    inv.set_profiling(True)
    inv.get_profile()
    ts = []
    for _ in range(calls):
        fn()
        torch.cuda.synchronize()
        ts.append(sum(ms for ms, _ in inv.get_profile().values()))
    inv.set_profiling(False)
    return round(statistics.median(ts), 4)


def finish(row, orders, k, others):
    o = np.asarray(orders, np.int64)
    x_bytes = int((o * o).sum()) * 4
    row["x_bytes"] = x_bytes
    row["bytes_x_r_z"] = x_bytes + 2 * int(o.sum()) * k * 4
    row["apply_gb_per_s"] = round(row["bytes_x_r_z"] / (row["apply"]["ms"] * 1e-3) / 1e9, 1)
    row["apply_kernels_gb_per_s"] = round(row["bytes_x_r_z"] / (row["apply_kernels_ms"] * 1e-3) / 1e9, 1)
    row["x_fits_infinity_cache"] = x_bytes <= INFINITY_CACHE_BYTES
    for other in others:
        row[f"apply_over_{other}"] = round(row["apply"]["ms"] / row[other]["ms"], 3)
        row[f"apply_slower_than_{other}"] = row["apply"]["ms"] > row[other]["ms"]


def measure_packed(torch, members, lo, hi, k, warmup, calls):
    orders, by_order = make_members(members, lo, hi)
    rng = np.random.default_rng(77 + k)
    slot = {int(i): (n, j) for n in by_order for j, i in enumerate(np.nonzero(orders == n)[0])}
    r_by_order = {n: rng.uniform(-1, 1, (len(a), n, k)).astype(np.float32) for n, a in by_order.items()}
    flat = np.concatenate([by_order[slot[i][0]][slot[i][1]].reshape(-1) for i in range(members)])
    r = np.concatenate([r_by_order[slot[i][0]][slot[i][1]] for i in range(members)])
    inv = g.Inverter()
    try:
        plan = inv.plan_ragged(orders)
        ta, tr = torch.from_numpy(flat).cuda(), torch.from_numpy(r).cuda()
        x_flat, st = inv.inv_ragged(plan, ta)          # set up once
        z, zs = torch.empty_like(tr), torch.empty_like(tr)
        sst = torch.empty(members, dtype=torch.int32, device="cuda")
        # the stored inverses grouped by order, for the bmm leg
        groups = []
        for n, a in by_order.items():
            gi, gst = inv.inv(torch.from_numpy(a).cuda())
            rr = torch.from_numpy(r_by_order[n]).cuda()
            groups.append((gi, rr, torch.empty_like(rr)))

        def bmm():
            for gi, rr, zz in groups:
                torch.bmm(gi, rr, out=zz)

        row = {"shape": "packed", "members": members, "orders": [int(orders.min()), int(orders.max())],
               "distinct_orders": len(by_order), "nrhs": k, "dtype": "float32",
               "apply_launches": len(inv.resolved_apply_ragged(orders, k)),
               "solve_launches": len(inv.resolved_solve_ragged(orders, k)), "bmm_calls": len(groups)}
        row.update(timed(torch, {"apply": lambda: inv.apply_ragged(plan, x_flat, tr, out=z),
                                 "solve": lambda: inv.solve_ragged(plan, ta, tr, out=zs, status=sst),
                                 "bmm": bmm}, warmup, calls))
        row["apply_kernels_ms"] = kernel_ms(torch, inv, lambda: inv.apply_ragged(plan, x_flat, tr, out=z), calls)
        finish(row, orders, k, ("solve", "bmm"))
        row["nonzero_status"] = int((st != 0).sum()) + int((sst != 0).sum())
        row["max_abs_difference_apply_solve"] = float((z - zs).abs().max())
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
        packed, st = inv.inv_diag_blocks(tm, orders, packed=True)     # set up once
        dense, _ = inv.inv_diag_blocks(tm, orders)
        z, zs, zd = torch.empty_like(tr), torch.empty_like(tr), torch.empty_like(tr)
        row = {"shape": "diagonal blocks", "matrix_order": DIAG_N, "members": len(orders),
               "orders": [min(orders), max(orders)], "nrhs": k, "dtype": "float32",
               "apply_launches": len(inv.resolved_apply_ragged(orders, k)),
               "solve_launches": len(inv.resolved_solve_ragged(orders, k)),
               "dense_bytes": DIAG_N * DIAG_N * 4}
        row.update(timed(torch, {"apply": lambda: inv.apply_diag_blocks(packed, orders, tr, out=z),
                                 "solve": lambda: inv.solve_diag_blocks(tm, orders, tr, out=zs),
                                 "dense": lambda: torch.matmul(dense, tr, out=zd)}, warmup, calls))
        row["apply_kernels_ms"] = kernel_ms(torch, inv, lambda: inv.apply_diag_blocks(packed, orders, tr, out=z), calls)
        finish(row, orders, k, ("solve", "dense"))
        row["nonzero_status"] = int((st != 0).sum())
        row["max_abs_difference_apply_dense"] = float((z - zd).abs().max())
    finally:
        inv.close()
    return row


def show(row):
    others = [o for o in ("solve", "bmm", "dense") if o in row]
    legs = " | ".join(f"{o} {row[o]['ms']:8.3f} ms (apply x{row['apply_over_' + o]:.3f}"
                      f"{', SLOWER' if row['apply_slower_than_' + o] else ''})" for o in others)
    print(f"{row['shape']:15s} members={row['members']:6d} orders {row['orders'][0]:3d}...{row['orders'][1]:3d} "
          f"K={row['nrhs']} apply {row['apply']['ms']:8.3f} ms ({row['apply_launches']} launches, "
          f"{row['apply_gb_per_s']:7.1f} GB/s; its kernels {row['apply_kernels_ms']:.3f} ms, "
          f"{row['apply_kernels_gb_per_s']:7.1f} GB/s; X {row['x_bytes'] / 2 ** 20:6.1f} MiB"
          f"{' fits' if row['x_fits_infinity_cache'] else ' exceeds'} the Infinity Cache) | {legs}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "apply", "ragged_apply.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--commit", default=None, help="what to record as the commit measured (default: git HEAD)")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("ragged_apply_bench.py needs a GPU; there is no fallback")
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
                     "torch.cuda.synchronize() around each call, device-resident tensors, one process; the same "
                     "inverses are re-read by every call (the Krylov case), so an X that fits the 256 MB Infinity "
                     "Cache is served from it",
           "hbm_spec_tb_per_s": HBM_SPEC_TBS, "device_copy_tb_per_s": COPY_TBS,
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
