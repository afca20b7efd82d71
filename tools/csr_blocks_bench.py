#!/usr/bin/env python3
"""The diagonal blocks of a CSR matrix gathered on the device: what ``Inverter.csr_diag_blocks`` / ``inv_csr_blocks``
cost against the ways a caller had before.

Shapes, fp32 values, int32 and int64 indices, generated from a seed: a 27-point stencil on a 3-D grid (27 entries per
row but at the faces, the columns of a row in a fixed shuffled order), values U(-1, 1) with 27 added on the diagonal,

* N = 2^20 rows (128 x 128 x 64), consecutive blocks of mixed orders 3 ... 64
* the same matrix, uniform order 32
* N = 2^18 rows (64 x 64 x 64), orders 65 ... 128
* N = 16 384 rows (32 x 32 x 16), orders 3 ... 64: the one size at which a dense copy fits

Per shape, in this one process and on the same device-resident data, alternating between the legs call by call (3
warm-up rounds, then the median of 7, min ... max recorded), each call between two device events on the stream:

* ``extract``      -- (a) ``csr_diag_blocks`` into a preallocated packed tensor
* ``extract_inv``  -- (b) ``inv_csr_blocks``: the gather, then ``inv_ragged`` in place
* ``torch``        -- (c) the gather in torch index arithmetic: row ids by ``repeat_interleave``, a mask on ``col``,
  ``index_put_`` into zeros (what depends on the block structure alone -- first row, order and packed offset per row --
  is computed once, outside the timed region)
* ``dense_inv``    -- (d) N = 16 384 only: ``to_dense()``, then ``inv_diag_blocks(packed=True)``

For ``extract`` the bytes the algorithm needs are computed from the shape -- row_ptr, col and val of the blocks' rows,
once, plus the ``sum n_b^2`` elements written -- and set over the time, beside the 6.29 TB/s a device-to-device copy
reaches on this part: the gather does no arithmetic, so memory traffic is the bound that applies.  Beside the call the
time of its kernels alone is reported (the context's event timing around each launch).  No threshold is asserted: a shape
on which the one call is slower than the torch leg is reported as such.

Prints a table and writes ``profiles/csr/csr_blocks.json`` (``--out``).  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gpu_matrix_inversion_amd as g  # noqa: E402
from gpu_matrix_inversion_amd import _lib  # noqa: E402

#         name                 grid            lowest, highest order   dense leg
SHAPES = (("mixed 3...64", (128, 128, 64), 3, 64, False),
          ("uniform 32", (128, 128, 64), 32, 32, False),
          ("orders 65...128", (64, 64, 64), 65, 128, False),
          ("dense fits", (32, 32, 16), 3, 64, True))
COPY_TBS = 6.29
DEVICE = "cuda"
HBM_SPEC_TBS = 8.0


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return None


def block_orders(n, lo, hi, seed):
    """Orders lo ... hi from a seed that sum to n (the last one is cut to fit)."""
    rng = np.random.default_rng(seed)
    orders = rng.integers(lo, hi + 1, n // lo + 1)
    keep = int(np.searchsorted(np.cumsum(orders), n)) + 1
    orders = orders[:keep].copy()
    orders[-1] -= int(orders.sum()) - n
    assert orders.sum() == n and orders.min() >= 1
    return orders


def stencil_csr(torch, grid, index_dtype, seed):
    """(crow, col, values) of the 27-point stencil on the grid, on the device."""
    nx, ny, nz = grid
    n = nx * ny * nz
    gen = torch.Generator(device=DEVICE).manual_seed(seed)
    row = torch.arange(n, device=DEVICE)
    x, y, z = row % nx, (row // nx) % ny, row // (nx * ny)
    steps = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    steps = [steps[i] for i in np.random.default_rng(seed).permutation(27)]          # unsorted columns
    cols, ok = [], []
    for dx, dy, dz in steps:
        inside = (x + dx >= 0) & (x + dx < nx) & (y + dy >= 0) & (y + dy < ny) & (z + dz >= 0) & (z + dz < nz)
        cols.append(row + dx + nx * dy + nx * ny * dz)
        ok.append(inside)
    cols, ok = torch.stack(cols, 1), torch.stack(ok, 1)
    crow = torch.zeros(n + 1, dtype=torch.int64, device=DEVICE)
    crow[1:] = ok.sum(1).cumsum(0)
    col = cols[ok]
    val = torch.rand(col.numel(), generator=gen, device=DEVICE) * 2 - 1
    val[col == row.unsqueeze(1).expand(-1, 27)[ok]] += 27.0
    return crow.to(index_dtype), col.to(index_dtype), val


def timed(torch, legs, warmup, calls):
    ts = {name: [] for name in legs}
    for i in range(warmup + calls):
        for name, fn in legs.items():   # alternating: a drift of the box hits every leg alike
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            if i >= warmup:
                ts[name].append(start.elapsed_time(stop))
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


def torch_leg(torch, crow, col, val, orders):
    """(the gather in torch index arithmetic as a callable, the list its packed result is left in).  What depends on
    the block structure alone, per row, is computed here, once."""
    n = crow.numel() - 1
    o64 = np.asarray(orders, np.int64)
    flat = int((o64 * o64).sum())
    order_of = torch.from_numpy(o64).to(DEVICE)
    blk = torch.repeat_interleave(torch.arange(len(o64), device=DEVICE), order_of)
    first = torch.from_numpy(np.concatenate(([0], np.cumsum(o64)[:-1]))).to(DEVICE)
    off = torch.from_numpy(np.concatenate(([0], np.cumsum(o64 * o64)[:-1]))).to(DEVICE)
    first_of_row, order_of_row = first[blk], order_of[blk]
    row_base = off[blk] + (torch.arange(n, device=DEVICE) - first_of_row) * order_of_row
    result = [None]

    def gather():
        rows = torch.repeat_interleave(torch.arange(n, device=DEVICE), (crow[1:] - crow[:-1]).long())
        c = col.long() - first_of_row[rows]
        m = (c >= 0) & (c < order_of_row[rows])
        out = torch.zeros(flat, dtype=val.dtype, device=DEVICE)
        out.index_put_((row_base[rows[m]] + c[m],), val[m])
        result[0] = out

    return gather, result


def measure(torch, name, grid, lo, hi, dense_leg, index_dtype, warmup, calls):
    crow, col, val = stencil_csr(torch, grid, index_dtype, 11)
    n = crow.numel() - 1
    orders = block_orders(n, lo, hi, 12)
    o64 = orders.astype(np.int64)
    flat = int((o64 * o64).sum())
    torch_gather, torch_out = torch_leg(torch, crow, col, val, orders)

    inv = g.Inverter()
    try:
        out = torch.empty(flat, device=DEVICE)
        legs = {"extract": lambda: inv.csr_diag_blocks((crow, col, val), orders, out=out),
                "extract_inv": lambda: inv.inv_csr_blocks((crow, col, val), orders),
                "torch": torch_gather}
        if dense_leg:
            a = torch.sparse_csr_tensor(crow, col, val, size=(n, n))
            legs["dense_inv"] = lambda: inv.inv_diag_blocks(a.to_dense(), orders, packed=True)
        row = {}
        if dense_leg:
            try:                        # torch's CSR support is in beta: a conversion it refuses is recorded, not fatal
                legs["dense_inv"]()
                torch.cuda.synchronize()
            except Exception as e:      # noqa: BLE001
                del legs["dense_inv"]
                row["dense_inv"] = f"not measured: {type(e).__name__}: {e}"
        row.update({"shape": name, "rows": n, "grid": list(grid), "nnz": col.numel(), "members": len(orders),
               "orders": [int(orders.min()), int(orders.max())], "dtype": "float32",
               "index_dtype": str(index_dtype).replace("torch.", ""), "packed_elements": flat,
               "launches": len(inv.resolved_apply_ragged(orders, 1))})
        row.update(timed(torch, legs, warmup, calls))
        row["extract_kernels_ms"] = kernel_ms(torch, inv, legs["extract"], calls)
        ib = crow.element_size()
        row["bytes_needed"] = (n + 1) * ib + col.numel() * (ib + 4) + flat * 4
        for leg in ("extract", "extract_kernels"):
            ms = row[leg]["ms"] if leg == "extract" else row["extract_kernels_ms"]
            row[f"{leg}_gb_per_s"] = round(row["bytes_needed"] / (ms * 1e-3) / 1e9, 1)
            row[f"{leg}_share_of_copy_rate"] = round(row[f"{leg}_gb_per_s"] / (COPY_TBS * 1e3), 3)
        row["extract_over_torch"] = round(row["extract"]["ms"] / row["torch"]["ms"], 3)
        row["extract_slower_than_torch"] = row["extract"]["ms"] > row["torch"]["ms"]
        if "dense_inv" in legs:
            row["extract_inv_over_dense_inv"] = round(row["extract_inv"]["ms"] / row["dense_inv"]["ms"], 3)
        # the legs computed the same blocks
        inv.csr_diag_blocks((crow, col, val), orders, out=out)
        torch_gather()
        torch.cuda.synchronize()
        row["torch_leg_equal"] = bool(torch.equal(out, torch_out[0]))
        x, st = inv.inv_csr_blocks((crow, col, val), orders)
        row["nonzero_status"] = int((st != 0).sum())
    finally:
        inv.close()
    return row


def show(row):
    dense = row.get("dense_inv")
    extra = "" if dense is None else f" | dense_inv {dense['ms']:8.3f} ms" if isinstance(dense, dict) else f" | dense_inv {dense}"
    print(f"{row['shape']:16s} N={row['rows']:8d} {row['index_dtype']:5s} members={row['members']:6d} "
          f"extract {row['extract']['ms']:7.3f} ms ({row['launches']} launches, {row['extract_gb_per_s']:7.1f} GB/s; its "
          f"kernels {row['extract_kernels_ms']:.3f} ms, {row['extract_kernels_gb_per_s']:7.1f} GB/s = "
          f"{100 * row['extract_kernels_share_of_copy_rate']:.1f}% of the copy rate) | extract_inv "
          f"{row['extract_inv']['ms']:8.3f} ms | torch {row['torch']['ms']:8.3f} ms (extract x{row['extract_over_torch']:.3f}"
          f"{', SLOWER' if row['extract_slower_than_torch'] else ''}){extra} | equal {row['torch_leg_equal']}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csr", "csr_blocks.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--commit", default=None, help="what to record as the commit measured (default: git HEAD)")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("csr_blocks_bench.py needs a GPU; there is no fallback")
    torch.cuda.set_device(0)
    rows = []
    for name, grid, lo, hi, dense_leg in SHAPES:
        for index_dtype in (torch.int32, torch.int64):
            rows.append(measure(torch, name, grid, lo, hi, dense_leg, index_dtype, args.warmup, args.calls))
            show(rows[-1])
    doc = {"device": torch.cuda.get_device_name(0), "commit": args.commit or commit(),
           "library_version": _lib.load().mi32_version(),
           "method": f"median of {args.calls} calls after {args.warmup} warm-ups, the legs alternating call by call, each "
                     "call between two device events on the stream, device-resident tensors, one process; "
                     "bytes_needed = row_ptr + col + val of the blocks' rows, once, plus the packed elements written",
           "hbm_spec_tb_per_s": HBM_SPEC_TBS, "device_copy_tb_per_s": COPY_TBS,
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
