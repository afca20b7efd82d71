#!/usr/bin/env python3
"""z = blockdiag(X) r from inverses stored in reduced precision: what ``Inverter.apply_stored`` costs beside
``Inverter.apply_ragged`` on the same members in the same run.

Shapes (the method of tools/ragged_apply_bench.py: 3 warm-up rounds, then the median of 7, the legs alternating call
by call, min ... max recorded, kernel time from the context's events beside the call time):

* the packed shapes of tools/ragged_apply_bench.py -- 16 384 members of orders 3 ... 64 and 4 096 members of orders
  65 ... 127 -- at K = 1 and K = 4, in fp32 (stores: native, float16, bfloat16) and fp64 (native, float32, float16)
* one shape that cannot fit the 256 MiB Infinity Cache: fp64, 32 768 members of order 64 at K = 1 and K = 4 -- 1 GiB
  native, 512 MiB as float32, 256 MiB as float16 (``--skip-large`` leaves it out)

Every store holds ALL members in the one format named (forced, not chosen by ``choose_storage``: this measures the
kernel, not the rule); the values are whatever the narrowing makes of the inverses.  ``apply_ragged`` is unchanged code,
so its leg is the parent commit's number.  For every leg the bytes of X (as stored) + R + Z over the call time and over
the kernel time are reported beside the 6.29 TB/s of a device copy.  No threshold is asserted: a store that is slower
than ``apply_ragged`` is reported as such.

Prints a table and writes ``profiles/stored/stored_apply.json`` (``--out``).  Needs a GPU: there is no fallback.
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

SHAPES = ((16_384, 3, 64), (4_096, 65, 128))   # members, lowest order, highest order (tools/ragged_apply_bench.py)
MAX_ORDER = 127
LARGE = (32_768, 64)                            # members, order: fp64, 1 GiB native
STORES = {"float32": (("native", 0), ("float16", 2), ("bfloat16", 3)),
          "float64": (("native", 0), ("float32", 1), ("float16", 2))}
COPY_TBS = 6.29
INFINITY_CACHE_BYTES = 256 * 2 ** 20


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return None


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
    """Median over `calls` calls of the time between the events that bracket the call's launches."""
    inv.set_profiling(True)
    inv.get_profile()
    ts = []
    for _ in range(calls):
        fn()
        torch.cuda.synchronize()
        ts.append(sum(ms for ms, _ in inv.get_profile().values()))
    inv.set_profiling(False)
    return round(statistics.median(ts), 4)


def measure(torch, orders, x_flat, dtype_name, k, warmup, calls, what):
    """One row: apply_ragged and one apply_stored leg per store of the dtype, on the device tensor x_flat."""
    inv = g.Inverter()
    try:
        plan = inv.plan_ragged(orders)
        gen = torch.Generator(device="cuda").manual_seed(77 + k)
        r = torch.rand((plan.total_rows, k), dtype=x_flat.dtype, device="cuda", generator=gen) * 2 - 1
        rz_bytes = 2 * r.numel() * r.element_size()
        z = torch.empty_like(r)
        legs = {"apply_ragged": lambda: inv.apply_ragged(plan, x_flat, r, out=z)}
        stores, outs = {}, {}
        for name, code in STORES[dtype_name]:
            stores[name] = inv.store_inverses(plan, x_flat, np.full(plan.batch, code, np.int32))
            outs[name] = torch.empty_like(r)
            legs[name] = (lambda s, o: lambda: inv.apply_stored(s, r, out=o))(stores[name], outs[name])
        row = {"shape": what, "members": int(plan.batch), "orders": [int(min(orders)), int(max(orders))], "nrhs": k,
               "dtype": dtype_name, "launches": len(inv.resolved_apply_ragged(orders, k, x_flat.element_size()))}
        row.update(timed(torch, legs, warmup, calls))
        for name, fn in legs.items():
            leg = row[name]
            leg["kernels_ms"] = kernel_ms(torch, inv, fn, calls)
            leg["x_bytes"] = x_flat.numel() * x_flat.element_size() if name == "apply_ragged" else stores[name].nbytes
            leg["bytes_x_r_z"] = leg["x_bytes"] + rz_bytes
            leg["gb_per_s"] = round(leg["bytes_x_r_z"] / (leg["ms"] * 1e-3) / 1e9, 1)
            leg["kernels_gb_per_s"] = round(leg["bytes_x_r_z"] / (leg["kernels_ms"] * 1e-3) / 1e9, 1)
            leg["kernels_share_of_copy"] = round(leg["kernels_gb_per_s"] / (COPY_TBS * 1e3), 3)
            leg["x_fits_infinity_cache"] = leg["x_bytes"] <= INFINITY_CACHE_BYTES
            if name != "apply_ragged":
                leg["over_apply_ragged"] = round(leg["ms"] / row["apply_ragged"]["ms"], 3)
                leg["kernels_over_apply_ragged"] = round(leg["kernels_ms"] / row["apply_ragged"]["kernels_ms"], 3)
                leg["slower_than_apply_ragged"] = leg["ms"] > row["apply_ragged"]["ms"]
        # the native store holds the same bits: so must Z
        row["native_equals_apply_ragged"] = bool(torch.equal(outs["native"].view(torch.uint8), z.view(torch.uint8)))
        plan.close()
    finally:
        inv.close()
    return row


def packed_inverses(torch, members, lo, hi, dtype):
    """(orders, the packed inverses on the device) of U(-1, 1) + sqrt(n) I members, the orders of
    tools/ragged_apply_bench.py."""
    orders = np.minimum(np.random.default_rng(9900 + members % 997 + hi).integers(lo, hi + 1, members), MAX_ORDER)
    rng = np.random.default_rng([9900 + members % 997 + hi, 1])
    flat = np.concatenate([(rng.uniform(-1, 1, (n, n)) + np.sqrt(n) * np.eye(n)).astype(dtype).reshape(-1) for n in orders])
    inv = g.Inverter()
    try:
        plan = inv.plan_ragged(orders)
        x, st = inv.inv_ragged(plan, torch.from_numpy(flat).cuda())
        assert not bool(st.any())
        plan.close()
    finally:
        inv.close()
    return orders, x


def large_inverses(torch, members, n):
    """(orders, packed fp64 'inverses' on the device) for the shape that exceeds the cache: generated on the device,
    diag ~ 1 / sqrt(n) plus small off-diagonal entries, inside every format's normal range.  Only the bytes matter."""
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand((members, n, n), dtype=torch.float64, device="cuda", generator=gen) * 0.02 + 0.001
    x += torch.eye(n, dtype=torch.float64, device="cuda") / np.sqrt(n)
    return np.full(members, n, np.int32), x.reshape(-1)


def show(row):
    base = row["apply_ragged"]
    print(f"{row['shape']:8s} {row['dtype']:7s} members={row['members']:6d} orders {row['orders'][0]:3d}...{row['orders'][1]:3d} "
          f"K={row['nrhs']} | apply_ragged {base['ms']:7.3f} ms (kernels {base['kernels_ms']:.3f} ms, "
          f"{base['kernels_gb_per_s']:7.1f} GB/s, X {base['x_bytes'] / 2 ** 20:6.1f} MiB)", flush=True)
    for name, _ in STORES[row["dtype"]]:
        leg = row[name]
        print(f"    stored {name:9s} {leg['ms']:7.3f} ms x{leg['over_apply_ragged']:.3f}"
              f"{' SLOWER' if leg['slower_than_apply_ragged'] else ''} (kernels {leg['kernels_ms']:.3f} ms "
              f"x{leg['kernels_over_apply_ragged']:.3f}, {leg['kernels_gb_per_s']:7.1f} GB/s = "
              f"{100 * leg['kernels_share_of_copy']:.0f} % of a copy, X {leg['x_bytes'] / 2 ** 20:6.1f} MiB"
              f"{' fits' if leg['x_fits_infinity_cache'] else ' exceeds'} the Infinity Cache)", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stored", "stored_apply.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--skip-large", action="store_true", help="leave out the 1 GiB shape")
    ap.add_argument("--commit", default=None, help="what to record as the commit measured (default: git HEAD)")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("stored_apply_bench.py needs a GPU; there is no fallback")
    torch.cuda.set_device(0)
    rows = []
    for dtype in (np.float32, np.float64):
        for members, lo, hi in SHAPES:
            orders, x = packed_inverses(torch, members, lo, hi, dtype)
            for k in (1, 4):
                rows.append(measure(torch, orders, x, np.dtype(dtype).name, k, args.warmup, args.calls, "packed"))
                show(rows[-1])
            del x
    if not args.skip_large:
        orders, x = large_inverses(torch, *LARGE)
        for k in (1, 4):
            rows.append(measure(torch, orders, x, "float64", k, args.warmup, args.calls, "large"))
            show(rows[-1])
        del x
    doc = {"device": torch.cuda.get_device_name(0), "commit": args.commit or commit(),
           "library_version": _lib.load().mi32_version(),
           "method": f"median of {args.calls} calls after {args.warmup} warm-ups, the legs alternating call by call, "
                     "torch.cuda.synchronize() around each call, device-resident tensors, one process; kernels_ms: the "
                     "context's event timing around the call's launches, median of the same number of calls; every "
                     "store holds all members in one forced format; the same inverses are re-read by every call (the "
                     "Krylov case), so an X that fits the 256 MiB Infinity Cache is served from it",
           "device_copy_tb_per_s": COPY_TBS, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
