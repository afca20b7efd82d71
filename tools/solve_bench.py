#!/usr/bin/env python3
"""A X = B on the one-launch batch paths: what ``Inverter.solve`` costs against the two ways a caller had before.

Shapes (N, K, batch): (8, 1, 16384), (32, 1, 4096), (32, 32, 4096), (64, 1, 2048) and (96, 4, 2048); fp32, partial
pivoting.  (64, 1) is the known cliff: the width 65 no longer fits a 64-lane group, so the member moves to a
256-thread workgroup.  Per shape, in this one process and on the same device-resident batch, alternating between the
legs call by call (3 warm-up rounds, then the median of 7):

* ``solve``        -- ``Inverter.solve``: one launch per chunk of columns, no inverse stored
* ``inv_bmm``      -- ``Inverter.inv`` under ``algo="resident"`` / ``"workgroup"`` followed by ``torch.bmm``: what a
  caller of this library had to do before (the inversion kernels are those of the commit before the solve: their code
  is unchanged by it)
* ``torch_solve``  -- ``torch.linalg.solve`` on the same batch (left out, with the reason, where it does not run on the
  box)

Each call is timed with a host clock between two ``torch.cuda.synchronize()``.  No threshold is asserted: a shape on
which ``solve`` is slower than ``inv_bmm`` is reported as such.  The forward errors of ``solve`` and ``inv_bmm`` against
``torch.linalg.solve`` on the float64 copy are reported where that runs.

Prints a table and writes ``profiles/solve/solve_batch.json`` (``--out``).  Needs a GPU: there is no fallback.
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

SHAPES = [(8, 1, 16_384), (32, 1, 4_096), (32, 32, 4_096), (64, 1, 2_048), (96, 4, 2_048)]


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return None


def make_batch(torch, n, k, batch):
    rng = np.random.default_rng(1000 * n + batch % 997)
    a = rng.uniform(-1, 1, (batch, n, n)).astype(np.float32)
    a += np.float32(np.sqrt(n)) * np.eye(n, dtype=np.float32)
    b = rng.uniform(-1, 1, (batch, n, k)).astype(np.float32)
    return torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()


def measure(torch, n, k, batch, warmup, calls):
    a, b = make_batch(torch, n, k, batch)
    algo = "resident" if n <= 64 else "workgroup"
    inv = g.Inverter(algo=algo)
    x = torch.empty_like(b)
    ainv = torch.empty_like(a)
    xb = torch.empty_like(b)
    st = torch.empty(batch, dtype=torch.int32, device=a.device)

    def inv_bmm():
        inv.inv(a, out=ainv, status=st)
        return torch.bmm(ainv, b, out=xb)

    legs = {"solve": lambda: inv.solve(a, b, out=x, status=st), "inv_bmm": inv_bmm}
    cols, launches, lanes, rows = inv.resolved_solve(n, k)
    row = {"n": n, "nrhs": k, "batch": batch, "dtype": "float32", "pivoting": True, "inv_algo": algo,
           "solve_launches": launches, "solve_kernel": f"resident, {lanes} lanes" if lanes else f"workgroup, {rows} rows"}
    try:
        torch.linalg.solve(a[:4], b[:4])
        torch.cuda.synchronize()
        legs["torch_solve"] = lambda: torch.linalg.solve(a, b)
    except Exception as e:  # the reason goes into the report
        row["torch_solve"] = f"not run: {type(e).__name__}: {e}"[:200]
    ts = {name: [] for name in legs}
    try:
        assert inv.resolved_algo(n, batch) == _lib.ALGO_NAMES[algo]
        for i in range(warmup + calls):
            for name, fn in legs.items():   # alternating: a drift of the box hits every leg alike
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if i >= warmup:
                    ts[name].append((time.perf_counter() - t0) * 1e3)
        _, st2 = inv.solve(a, b, out=x)
        inv_bmm()
        torch.cuda.synchronize()
    finally:
        inv.close()
    for name, v in ts.items():
        row[name] = {"ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    row["solve_over_inv_bmm"] = round(row["solve"]["ms"] / row["inv_bmm"]["ms"], 3)
    row["solve_slower_than_inv_bmm"] = row["solve"]["ms"] > row["inv_bmm"]["ms"]
    if "torch_solve" in ts:
        row["solve_over_torch_solve"] = round(row["solve"]["ms"] / row["torch_solve"]["ms"], 3)
    row["nonzero_status"] = int((st2 != 0).sum())
    try:
        ref = torch.linalg.solve(a.double(), b.double())
        torch.cuda.synchronize()
        scale = ref.abs().amax(dim=(1, 2))
        row["max_forward_error_solve"] = float(((x.double() - ref).abs().amax(dim=(1, 2)) / scale).max())
        row["max_forward_error_inv_bmm"] = float(((xb.double() - ref).abs().amax(dim=(1, 2)) / scale).max())
    except Exception as e:
        row["vs_torch_f64"] = f"not run: {type(e).__name__}: {e}"[:200]
    return row


def show(row):
    line = f"n={row['n']:3d} K={row['nrhs']:3d} B={row['batch']:6d} {row['solve_kernel']:19s} solve " \
           f"{row['solve']['ms']:8.3f} ms | inv + bmm {row['inv_bmm']['ms']:8.3f} ms (solve x{row['solve_over_inv_bmm']:.3f}" \
           f"{', SLOWER' if row['solve_slower_than_inv_bmm'] else ''})"
    p = row.get("torch_solve")
    line += f" | torch.linalg.solve {p['ms']:8.3f} ms" if isinstance(p, dict) else f" | torch.linalg.solve: {p}"
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solve", "solve_batch.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--commit", default=None, help="what to record as the commit measured (default: git HEAD)")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("solve_bench.py needs a GPU; there is no fallback")
    torch.cuda.set_device(0)
    rows = []
    for n, k, b in SHAPES:
        rows.append(measure(torch, n, k, b, args.warmup, args.calls))
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
