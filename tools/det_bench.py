#!/usr/bin/env python3
"""The determinant beside the inverse: what ``Inverter.inv_det`` costs over the plain inversion, and what it saves.

Shapes: the three timed shapes of the register-resident path (tests/resident_cases.py: 8 x 16384, 32 x 4096, 64 x 2048)
and 96 x 96 x 2048 for the workgroup-resident path; fp32, partial pivoting.  Per shape, in this one process and on the
same device-resident batch, alternating between the legs call by call (3 warm-up rounds, then the median of 7):

* ``inv``             -- the plain call under ``algo="resident"`` / ``"workgroup"``: the code before the determinant
* ``inv_det``         -- inverse and determinant from one launch
* ``det_only``        -- ``inv_det(want_inverse=False)``: status and determinant, no inverse stored
* ``inv_plus_slogdet``-- ``inv`` followed by ``torch.linalg.slogdet`` on the same batch: what a caller had to do
  before (left out, with the reason, where torch's slogdet does not run on the box)

Each call is timed with a host clock between two ``torch.cuda.synchronize()``.  The determinants are compared with
``torch.linalg.slogdet`` on the float64 copy of the batch where that runs (reported, not asserted).

Prints a table and writes ``profiles/det/det_batch.json`` (``--out``).  Needs a GPU: there is no fallback.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gpu_matrix_inversion_amd as g  # noqa: E402
from gpu_matrix_inversion_amd import _lib  # noqa: E402
from resident_cases import TIMED_SHAPES  # noqa: E402

WORKGROUP_SHAPE = (96, 2_048)


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return None


def make_batch(torch, n, batch):
    rng = np.random.default_rng(1000 * n + batch % 997)
    a = rng.uniform(-1, 1, (batch, n, n)).astype(np.float32)
    a += np.float32(np.sqrt(n)) * np.eye(n, dtype=np.float32)
    return torch.from_numpy(a).cuda()


def measure(torch, n, batch, warmup, calls):
    a = make_batch(torch, n, batch)
    algo = "resident" if n <= 64 else "workgroup"
    inv = g.Inverter(algo=algo)
    out = torch.empty_like(a)
    st = torch.empty(batch, dtype=torch.int32, device=a.device)
    legs = {"inv": lambda: inv.inv(a, out=out, status=st),
            "inv_det": lambda: inv.inv_det(a, out=out, status=st),
            "det_only": lambda: inv.inv_det(a, status=st, want_inverse=False)}
    row = {"n": n, "batch": batch, "dtype": "float32", "pivoting": True, "algo": algo}
    try:
        torch.linalg.slogdet(a[:4])
        torch.cuda.synchronize()

        def inv_plus_slogdet():
            inv.inv(a, out=out, status=st)
            return torch.linalg.slogdet(a)

        legs["inv_plus_slogdet"] = inv_plus_slogdet
    except Exception as e:  # the reason goes into the report
        row["inv_plus_slogdet"] = f"not run: {type(e).__name__}: {e}"[:200]
    ts = {k: [] for k in legs}
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
        plain, _ = inv.inv(a)
        x, st2, mant, exp = inv.inv_det(a)
        _, st3, mant3, exp3 = inv.inv_det(a, want_inverse=False)
        torch.cuda.synchronize()
    finally:
        inv.close()
    for name, v in ts.items():
        row[name] = {"ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    base = row["inv"]["ms"]
    row["inv_det_over_inv"] = round(row["inv_det"]["ms"] / base, 3)
    row["det_only_over_inv"] = round(row["det_only"]["ms"] / base, 3)
    if "inv_plus_slogdet" in ts:
        row["inv_plus_slogdet_over_inv_det"] = round(row["inv_plus_slogdet"]["ms"] / row["inv_det"]["ms"], 3)
    row["nonzero_status"] = int((st2 != 0).sum())
    row["same_inverse_as_inv"] = bool(torch.equal(x, plain))
    row["det_only_same_pair"] = bool(torch.equal(st2, st3) and torch.equal(exp, exp3)
                                     and torch.equal(mant.view(torch.int64), mant3.view(torch.int64)))
    try:
        sign, logabs = g.slogdet_from_frexp(mant, exp)
        ref = torch.linalg.slogdet(a.double())
        torch.cuda.synchronize()
        row["sign_mismatches_vs_torch_f64"] = int((sign != ref.sign).sum())
        row["max_logabsdet_diff_vs_torch_f64"] = float((logabs - ref.logabsdet).abs().max())
    except Exception as e:
        row["vs_torch_f64"] = f"not run: {type(e).__name__}: {e}"[:200]
    return row


def show(row):
    line = f"n={row['n']:3d} B={row['batch']:6d} {row['algo']:9s} inv {row['inv']['ms']:8.3f} ms | inv_det " \
           f"{row['inv_det']['ms']:8.3f} ms (x{row['inv_det_over_inv']:.3f}) | det only {row['det_only']['ms']:8.3f} ms " \
           f"(x{row['det_only_over_inv']:.3f})"
    p = row.get("inv_plus_slogdet")
    line += f" | inv + torch slogdet {p['ms']:8.3f} ms" if isinstance(p, dict) else f" | inv + torch slogdet: {p}"
    line += f" | same inverse: {row['same_inverse_as_inv']}"
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "det", "det_batch.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--commit", default=None, help="what to record as the commit measured (default: git HEAD)")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("det_bench.py needs a GPU; there is no fallback")
    torch.cuda.set_device(0)
    rows = []
    for n, b in list(TIMED_SHAPES) + [WORKGROUP_SHAPE]:
        rows.append(measure(torch, n, b, args.warmup, args.calls))
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
