#!/usr/bin/env python3
"""One block-Jacobi relaxation sweep from the CSR matrix and the stored block inverses: what the fused
``Inverter.relax_stored`` costs against the chain of calls a caller had before, in the method of
tools/csr_blocks_bench.py (whose matrices and timing helpers this tool uses).

Shapes: the 27-point-stencil matrices of csr_blocks_bench.py, int32 indices --

* N = 2^20 rows, consecutive blocks of mixed orders 3 ... 64
* the same matrix, uniform order 32
* N = 2^18 rows, orders 65 ... 128
* N = 16 384 rows, orders 3 ... 64

-- each as fp32 with an all-native and an all-float16 store, and as fp64 with an all-float16 store.  The store is set
up once per case, outside the timed region (``inv_csr_blocks``, then ``store_inverses``).

Per case, in this one process and on the same device-resident data, alternating between the legs call by call (3
warm-up rounds, then the median of 7, min ... max recorded), each call between two device events on the stream:

* ``relax``     -- ``relax_stored`` with ``out=`` given: one launch per lane class
* ``chain``     -- the unfused sweep: ``torch.mv`` of the ``torch.sparse_csr`` matrix, a subtraction from b,
  ``apply_stored``, an addition to x
* ``residual``  -- ``csr_block_residual`` alone, ``out=`` given

Beside ``relax`` and ``residual`` the time of their kernels alone is reported (the context's event timing around each
launch).  The bytes a sweep needs -- the CSR arrays, x, b, the store and x', each once -- are set over the kernels'
time, beside the 6.29 TB/s a device-to-device copy reaches on this part.  The chain's result differs from the fused
one in the last bits (torch's product promises no summation order): the largest difference relative to the largest
|x'| is recorded, not asserted.  No speed-up is asserted either: a case on which the fused call is slower than the chain
is reported as such.

Prints a table and writes ``profiles/relax/relax.json`` (``--out``).  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gpu_matrix_inversion_amd as g  # noqa: E402
from gpu_matrix_inversion_amd import _lib  # noqa: E402
from csr_blocks_bench import COPY_TBS, DEVICE, HBM_SPEC_TBS, SHAPES, block_orders, commit, kernel_ms, stencil_csr, timed  # noqa: E402

NATIVE, FLOAT16 = 0, 2
#        working type, store format
CASES = (("float32", NATIVE), ("float32", FLOAT16), ("float64", FLOAT16))


def measure(torch, name, grid, lo, hi, dtype_name, code, warmup, calls):
    dtype = getattr(torch, dtype_name)
    crow, col, val = stencil_csr(torch, grid, torch.int32, 11)
    val = val.to(dtype)
    n = crow.numel() - 1
    orders = block_orders(n, lo, hi, 12)
    gen = torch.Generator(device=DEVICE).manual_seed(13)
    x = (torch.rand(n, generator=gen, device=DEVICE) * 2 - 1).to(dtype)
    b = (torch.rand(n, generator=gen, device=DEVICE) * 2 - 1).to(dtype)
    a = (crow, col, val)
    a_torch = torch.sparse_csr_tensor(crow, col, val, size=(n, n))

    inv = g.Inverter()
    try:
        packed, status = inv.inv_csr_blocks(a, orders)
        plan = inv._diag_blocks_plan(None, orders)[0]
        stored = inv.store_inverses(plan, packed, np.full(len(orders), code, np.int32))
        inv._diag_plan = None       # the store owns the plan now
        del packed
        out, rout = torch.empty_like(x), torch.empty_like(x)
        chain_out = [None]

        def chain():
            r = b - torch.mv(a_torch, x)
            chain_out[0] = x + inv.apply_stored(stored, r)

        legs = {"relax": lambda: inv.relax_stored(a, stored, x, b, 1.0, out=out),
                "chain": chain,
                "residual": lambda: inv.csr_block_residual(a, plan, x, b, out=rout)}
        es, ib = val.element_size(), crow.element_size()
        row = {"shape": name, "rows": n, "grid": list(grid), "nnz": col.numel(), "members": len(orders),
               "orders": [int(orders.min()), int(orders.max())], "dtype": dtype_name, "index_dtype": "int32",
               "store_format": {NATIVE: "native", FLOAT16: "float16"}[code], "store_bytes": stored.nbytes,
               "launches": len(inv.resolved_apply_ragged(orders, 1)), "nonzero_status": int((status != 0).sum())}
        row.update(timed(torch, legs, warmup, calls))
        row["relax_kernels_ms"] = kernel_ms(torch, inv, legs["relax"], calls)
        row["residual_kernels_ms"] = kernel_ms(torch, inv, legs["residual"], calls)
        row["bytes_needed"] = (n + 1) * ib + col.numel() * (ib + es) + 3 * n * es + stored.nbytes
        row["relax_kernels_gb_per_s"] = round(row["bytes_needed"] / (row["relax_kernels_ms"] * 1e-3) / 1e9, 1)
        row["relax_kernels_share_of_copy_rate"] = round(row["relax_kernels_gb_per_s"] / (COPY_TBS * 1e3), 3)
        row["relax_over_chain"] = round(row["relax"]["ms"] / row["chain"]["ms"], 3)
        row["relax_slower_than_chain"] = row["relax"]["ms"] > row["chain"]["ms"]
        # the legs computed the same sweep, up to the order of torch's sums
        legs["relax"]()
        chain()
        torch.cuda.synchronize()
        row["chain_max_difference_over_max"] = float((out - chain_out[0]).abs().max() / out.abs().max())
        plan.close()
    finally:
        inv.close()
    return row


def show(row):
    print(f"{row['shape']:16s} N={row['rows']:8d} {row['dtype']:7s} store {row['store_format']:7s} members={row['members']:6d} "
          f"relax {row['relax']['ms']:7.3f} ms ({row['launches']} launches; its kernels {row['relax_kernels_ms']:.3f} ms, "
          f"{row['relax_kernels_gb_per_s']:7.1f} GB/s = {100 * row['relax_kernels_share_of_copy_rate']:.1f}% of the copy "
          f"rate) | chain {row['chain']['ms']:7.3f} ms (relax x{row['relax_over_chain']:.3f}"
          f"{', SLOWER' if row['relax_slower_than_chain'] else ''}) | residual {row['residual']['ms']:7.3f} ms (kernels "
          f"{row['residual_kernels_ms']:.3f} ms) | chain differs by {row['chain_max_difference_over_max']:.1e}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relax", "relax.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--commit", default=None, help="what to record as the commit measured (default: git HEAD)")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("csr_relax_bench.py needs a GPU; there is no fallback")
    torch.cuda.set_device(0)
    rows = []
    for name, grid, lo, hi, _ in SHAPES:
        for dtype_name, code in CASES:
            rows.append(measure(torch, name, grid, lo, hi, dtype_name, code, args.warmup, args.calls))
            show(rows[-1])
    doc = {"device": torch.cuda.get_device_name(0), "commit": args.commit or commit(),
           "library_version": _lib.load().mi32_version(),
           "method": f"median of {args.calls} calls after {args.warmup} warm-ups, the legs alternating call by call, each "
                     "call between two device events on the stream, device-resident tensors, one process; "
                     "bytes_needed = row_ptr + col + val + x + b + the store + x', each once",
           "hbm_spec_tb_per_s": HBM_SPEC_TBS, "device_copy_tb_per_s": COPY_TBS,
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
