#!/usr/bin/env python3
"""The block-Jacobi blocks of a CSR sparsity pattern found on the device: what ``Inverter.csr_block_starts`` /
``csr_find_blocks`` cost against the only way a caller had before, the pattern copied to the host.

Shapes as in tools/csr_blocks_bench.py, generated from a seed: the 27-point stencil on a 3-D grid (27 entries per row
but at the faces, the columns of a row in a fixed shuffled order, so every row differs from the one before it and every
pair of interior rows is compared to its last entry) at N = 2^20, 2^18 and 16 384 rows, and a 64 x 64 x 32 grid with
3 unknowns per node (the rows of a node share the node's pattern, 243 entries: runs of 3); int32 and int64 indices;
``max_order`` 32 and 128, with agglomeration.

Per shape, in this one process and on the same device-resident data, alternating between the legs call by call (3
warm-up rounds, then the median of 7, min ... max recorded), each call between two device events on the stream:

* ``starts``  -- ``csr_block_starts`` into a preallocated output (the temporary memory is the call's ``torch.empty``)
* ``orders``  -- ``csr_find_blocks``: the same, the N-byte copy to the host, ``flatnonzero`` and ``diff``
* ``host``    -- ``crow.cpu()``, ``col.cpu()`` and the three steps of the definition vectorised in NumPy (the orbit is a
  loop over the blocks on a precomputed ``next``), copies included

``starts`` is then timed once more on its own, call after call (``starts_back_to_back``): in the alternation it follows
the host leg, during which the device has nothing to do.

Beside the call the time of its kernels alone (the context's event timing around the launches) and of each stage alone
(the stage launched by itself on the temporary memory a whole call left, between two events) are reported.  The bytes
the algorithm needs -- row_ptr and col once, the temporary memory and the output -- are set over the kernels' time,
beside the 6.29 TB/s a device-to-device copy reaches on this part.  No threshold is asserted: a shape on which the host
leg wins is reported as such.

Prints a table and writes ``profiles/csr/find_blocks.json`` (``--out``).  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gpu_matrix_inversion_amd as g  # noqa: E402
from gpu_matrix_inversion_amd import _lib, api  # noqa: E402
from csr_blocks_bench import COPY_TBS, DEVICE, HBM_SPEC_TBS, commit, kernel_ms, stencil_csr, timed  # noqa: E402

#         name                       grid        unknowns per node
SHAPES = (("stencil 2^20", (128, 128, 64), 1),
          ("stencil 2^18", (64, 64, 64), 1),
          ("stencil 16384", (32, 32, 16), 1),
          ("3 per node, 3 x 2^17", (64, 64, 32), 3))
STAGES = (("nat", 1), ("runs", 2), ("sv", 4), ("chain", 8), ("mark", 16))


def node_pattern(torch, crow, col, dof):
    """The pattern with ``dof`` unknowns per node: the rows of a node share the node's columns, each widened to the
    node's unknowns."""
    if dof == 1:
        return crow, col
    n = crow.numel() - 1
    lens = (crow[1:] - crow[:-1]).long()
    wide = (col.long().unsqueeze(1) * dof + torch.arange(dof, device=col.device)).reshape(-1)      # per node row
    node_start = crow[:-1].long() * dof
    rows = torch.repeat_interleave(torch.arange(n, device=col.device), dof)
    new_lens = lens[rows] * dof
    new_crow = torch.zeros(n * dof + 1, dtype=torch.int64, device=col.device)
    new_crow[1:] = new_lens.cumsum(0)
    # entry k of unknown row r of node i is entry k of the node's widened row
    k = torch.arange(int(new_crow[-1]), device=col.device) - torch.repeat_interleave(new_crow[:-1], new_lens)
    new_col = wide[torch.repeat_interleave(node_start[rows], new_lens) + k]
    return new_crow.to(crow.dtype), new_col.to(col.dtype)


def host_starts(crow, col, max_order, agglomerate):
    """The definition on the host, vectorised: what a caller without the device call does, copies included."""
    crow, col = crow.cpu().numpy().astype(np.int64), col.cpu().numpy()
    n = crow.size - 1
    lens = np.diff(crow)
    rows = np.repeat(np.arange(n), lens)
    same_len = np.zeros(n, bool)
    same_len[1:] = lens[1:] == lens[:-1]
    e = np.flatnonzero(same_len[rows])                              # the entries of rows as long as the row before
    differ = col[e] != col[e - lens[rows[e]]]                       # the same place in the row before
    nat = ~same_len
    nat[rows[e[differ]]] = True
    idx = np.arange(n)
    run = np.maximum.accumulate(np.where(nat, idx, 0))
    sv = nat | ((idx - run) % max_order == 0)
    if not agglomerate:
        return sv.astype(np.uint8)
    last = np.maximum.accumulate(np.where(np.append(sv, True), np.arange(n + 1), -1))
    nxt = last[np.minimum(idx + max_order, n)]
    start = np.zeros(n, np.uint8)
    i = 0
    while i < n:
        start[i] = 1
        i = int(nxt[i])
    return start


def stage_ms(torch, inv, crow, col, max_order, out, calls):
    """{stage: median ms} of every stage launched alone between two events, on the temporary memory of a whole call."""
    n = crow.numel() - 1
    nbytes = api.find_blocks_work_bytes(n)
    work = torch.empty(nbytes, dtype=torch.uint8, device=DEVICE)
    lib = _lib.load()
    args = (inv._h, n, api._ptr(crow), api._ptr(col), crow.element_size(), max_order, 1, api._ptr(out), api._ptr(work),
            nbytes)
    inv._bind_stream()
    _lib.check(lib.mi32_debug_csr_find_stages(*args, 31), "whole call")
    res = {}
    for name, bit in STAGES:
        ts = []
        for i in range(3 + calls):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            _lib.check(lib.mi32_debug_csr_find_stages(*args, bit), name)
            stop.record()
            stop.synchronize()
            if i >= 3:
                ts.append(start.elapsed_time(stop))
        res[name] = round(statistics.median(ts), 4)
    return res


def measure(torch, name, grid, dof, index_dtype, max_order, warmup, calls):
    crow, col, _ = stencil_csr(torch, grid, index_dtype, 11)
    crow, col = node_pattern(torch, crow, col, dof)
    n = crow.numel() - 1
    a = (crow, col, None)
    inv = g.Inverter()
    try:
        out = torch.empty(n, dtype=torch.uint8, device=DEVICE)
        host_out = [None]

        def host_leg():
            host_out[0] = host_starts(crow, col, max_order, True)

        legs = {"starts": lambda: inv.csr_block_starts(a, max_order, out=out),
                "orders": lambda: inv.csr_find_blocks(a, max_order),
                "host": host_leg}
        ib = crow.element_size()
        work = api.find_blocks_work_bytes(n)
        row = {"shape": name, "rows": n, "grid": list(grid), "unknowns_per_node": dof, "nnz": col.numel(),
               "index_dtype": str(index_dtype).replace("torch.", ""), "max_order": max_order, "agglomerate": True,
               "work_bytes": work, "work_bytes_per_row": round(work / n, 3)}
        row.update(timed(torch, legs, warmup, calls))
        # the same call again with no host leg between the calls: the 0.3 s of host work leave the device idle
        row["starts_back_to_back"] = timed(torch, {"starts": legs["starts"]}, warmup, calls)["starts"]
        row["kernels_ms"] = kernel_ms(torch, inv, legs["starts"], calls)
        row["stage_ms"] = stage_ms(torch, inv, crow, col, max_order, out, calls)
        row["bytes_needed"] = (n + 1) * ib + col.numel() * ib + work + n
        row["kernels_gb_per_s"] = round(row["bytes_needed"] / (row["kernels_ms"] * 1e-3) / 1e9, 1)
        row["kernels_share_of_copy_rate"] = round(row["kernels_gb_per_s"] / (COPY_TBS * 1e3), 3)
        row["nat_gb_per_s"] = round(((n + 1) * ib + col.numel() * ib + n) / (row["stage_ms"]["nat"] * 1e-3) / 1e9, 1)
        row["behind_nat_over_nat"] = round(sum(v for k, v in row["stage_ms"].items() if k != "nat") / row["stage_ms"]["nat"], 3)
        row["starts_over_host"] = round(row["starts"]["ms"] / row["host"]["ms"], 4)
        row["host_wins"] = row["host"]["ms"] < row["orders"]["ms"]
        inv.csr_block_starts(a, max_order, out=out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        row["host_leg_equal"] = bool(np.array_equal(got, host_out[0]))
        orders = np.diff(np.flatnonzero(got), append=n)
        row["blocks"] = int(orders.size)
        row["orders"]["range"] = [int(orders.min()), int(orders.max())]
    finally:
        inv.close()
    return row


def show(row):
    st = row["stage_ms"]
    print(f"{row['shape']:22s} N={row['rows']:8d} {row['index_dtype']:5s} max_order={row['max_order']:3d} "
          f"blocks={row['blocks']:7d} | starts {row['starts']['ms']:7.3f} ms, back to back {row['starts_back_to_back']['ms']:.3f} ms (kernels {row['kernels_ms']:.3f} ms, "
          f"{row['kernels_gb_per_s']:7.1f} GB/s = {100 * row['kernels_share_of_copy_rate']:.1f}% of the copy rate; "
          + " ".join(f"{k} {v:.3f}" for k, v in st.items()) + f") | orders {row['orders']['ms']:7.3f} ms | host "
          f"{row['host']['ms']:9.3f} ms{' HOST WINS' if row['host_wins'] else ''} | equal {row['host_leg_equal']}",
          flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csr", "find_blocks.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--commit", default=None, help="what to record as the commit measured (default: git HEAD)")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("csr_find_blocks_bench.py needs a GPU; there is no fallback")
    torch.cuda.set_device(0)
    rows = []
    for name, grid, dof in SHAPES:
        for index_dtype in (torch.int32, torch.int64):
            for max_order in (32, 128):
                rows.append(measure(torch, name, grid, dof, index_dtype, max_order, args.warmup, args.calls))
                show(rows[-1])
    doc = {"device": torch.cuda.get_device_name(0), "commit": args.commit or commit(),
           "library_version": _lib.load().mi32_version(),
           "method": f"median of {args.calls} calls after {args.warmup} warm-ups, the legs alternating call by call, each "
                     "call between two device events on the stream, device-resident tensors, one process; stage_ms: the "
                     "stage launched alone on the temporary memory of a whole call; bytes_needed = row_ptr + col once, "
                     "the temporary memory and the output",
           "hbm_spec_tb_per_s": HBM_SPEC_TBS, "device_copy_tb_per_s": COPY_TBS,
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
