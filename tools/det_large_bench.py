#!/usr/bin/env python3
"""The determinant beside the inverse above order 128: what ``Inverter.inv_det_any`` costs over the plain inversion on
the sweep / blocked paths, and what it saves over ``inv`` followed by ``torch.linalg.slogdet``.

Shapes: fp32 with pivoting at N = 2048 (batch 1 and 8), 4096 and 16384; fp64 at N = 4096 with pivoting and without.
Per shape, in this one process and on the same device-resident batch, alternating between the legs call by call
(3 warm-up rounds, then the median of 7, with min ... max):

* ``inv``              -- the plain call: the code before this feature
* ``inv_det_any``      -- inverse and determinant from the same elimination
* ``det_only``         -- ``inv_det_any(want_inverse=False)``: status and determinant, no inverse stored
* ``inv_plus_slogdet`` -- ``inv`` followed by ``torch.linalg.slogdet`` on the same batch: what a caller had to do
  before (left out, with the reason, where torch's slogdet does not run on the box)

Each call is timed with a host clock between two ``torch.cuda.synchronize()``.  After the timed rounds one ``inv`` and
one ``inv_det_any`` run under the library's per-class event profiler (``get_profile``): the added launches are
accounted to the ``finish`` class, so the difference of that class is what the determinant adds on the device.  The
differences of sign and logabsdet from ``torch.linalg.slogdet`` on the float64 copy are reported, not asserted.

Prints a table and writes ``profiles/det/det_large.json`` (``--out``).  Needs a GPU: there is no fallback.
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

# (n, batch, dtype, pivoting)
SHAPES = [(2048, 1, "float32", True), (2048, 8, "float32", True), (4096, 1, "float32", True), (16384, 1, "float32", True),
          (4096, 1, "float64", True), (4096, 1, "float64", False)]


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return None


def make_batch(torch, n, batch, dtype, pivoting):
    rng = np.random.default_rng(1000 * n + batch % 997)
    a = rng.uniform(-1, 1, (batch, n, n)).astype(dtype)
    if pivoting:
        a += np.sqrt(n).astype(dtype) * np.eye(n, dtype=dtype)
        for b in range(batch):
            a[b] = a[b][rng.permutation(n)]  # rows shuffled: about n exchanging steps
    else:
        idx = np.arange(n)
        a[:, idx, idx] = np.abs(a).sum(axis=2) + 1.0  # strictly diagonally dominant
    return torch.from_numpy(a).cuda()


def measure(torch, n, batch, dtype, pivoting, warmup, calls):
    a = make_batch(torch, n, batch, dtype, pivoting)
    inv = g.Inverter(pivoting=pivoting)
    out = torch.empty_like(a)
    st = torch.empty(batch, dtype=torch.int32, device=a.device)
    legs = {"inv": lambda: inv.inv(a, out=out, status=st),
            "inv_det_any": lambda: inv.inv_det_any(a, out=out, status=st),
            "det_only": lambda: inv.inv_det_any(a, status=st, want_inverse=False)}
    row = {"n": n, "batch": batch, "dtype": dtype, "pivoting": pivoting}
    try:
        torch.linalg.slogdet(a[:, :64, :64])
        torch.cuda.synchronize()

        def inv_plus_slogdet():
            inv.inv(a, out=out, status=st)
            return torch.linalg.slogdet(a)

        legs["inv_plus_slogdet"] = inv_plus_slogdet
    except Exception as e:  # the reason goes into the report
        row["inv_plus_slogdet"] = f"not run: {type(e).__name__}: {e}"[:200]
    ts = {k: [] for k in legs}
    try:
        for i in range(warmup + calls):
            for name, fn in legs.items():   # alternating: a drift of the box hits every leg alike
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if i >= warmup:
                    ts[name].append((time.perf_counter() - t0) * 1e3)
        plain, _ = inv.inv(a)
        x, st2, mant, exp = inv.inv_det_any(a)
        _, st3, mant3, exp3 = inv.inv_det_any(a, want_inverse=False)
        torch.cuda.synchronize()
        # per kernel class, one call each (event pairs around every launch: the calls themselves run slower)
        inv.set_profiling(True)
        inv.inv(a, out=out, status=st)
        torch.cuda.synchronize()
        prof_inv = inv.get_profile()
        inv.inv_det_any(a, out=out, status=st)
        torch.cuda.synchronize()
        prof_det = inv.get_profile()
        inv.set_profiling(False)
    finally:
        inv.close()
    for name, v in ts.items():
        row[name] = {"ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    base = row["inv"]["ms"]
    row["inv_det_any_over_inv"] = round(row["inv_det_any"]["ms"] / base, 4)
    row["det_only_over_inv"] = round(row["det_only"]["ms"] / base, 4)
    row["inv_det_any_minus_inv_ms"] = round(row["inv_det_any"]["ms"] - base, 4)
    row["inv_spread_ms"] = round(row["inv"]["max_ms"] - row["inv"]["min_ms"], 4)
    if "inv_plus_slogdet" in ts:
        row["inv_plus_slogdet_over_inv_det_any"] = round(row["inv_plus_slogdet"]["ms"] / row["inv_det_any"]["ms"], 3)
    row["profile_ms_launches"] = {k: {"inv": [round(prof_inv[k][0], 4), prof_inv[k][1]],
                                      "inv_det_any": [round(prof_det[k][0], 4), prof_det[k][1]]}
                                  for k in prof_inv if prof_inv[k][1] or prof_det[k][1]}
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
        row["logabsdet"] = float(logabs[0])
    except Exception as e:
        row["vs_torch_f64"] = f"not run: {type(e).__name__}: {e}"[:200]
    return row


def show(row):
    line = f"n={row['n']:5d} B={row['batch']:2d} {row['dtype']} piv={int(row['pivoting'])} inv {row['inv']['ms']:9.3f} ms " \
           f"[{row['inv']['min_ms']:.3f} ... {row['inv']['max_ms']:.3f}] | inv_det_any {row['inv_det_any']['ms']:9.3f} ms " \
           f"(x{row['inv_det_any_over_inv']:.4f}) | det only {row['det_only']['ms']:9.3f} ms (x{row['det_only_over_inv']:.4f})"
    p = row.get("inv_plus_slogdet")
    line += f" | inv + torch slogdet {p['ms']:9.3f} ms" if isinstance(p, dict) else f" | inv + torch slogdet: {p}"
    line += f" | same inverse: {row['same_inverse_as_inv']} | finish class " \
            f"{row['profile_ms_launches'].get('finish')}"
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "det", "det_large.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--commit", default=None, help="what to record as the commit measured (default: git HEAD)")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("det_large_bench.py needs a GPU; there is no fallback")
    torch.cuda.set_device(0)
    rows = []
    for n, b, dtype, piv in SHAPES:
        rows.append(measure(torch, n, b, dtype, piv, args.warmup, args.calls))
        show(rows[-1])
    doc = {"device": torch.cuda.get_device_name(0), "commit": args.commit or commit(),
           "library_version": _lib.load().mi32_version(),
           "method": f"median of {args.calls} calls after {args.warmup} warm-ups, the legs alternating call by call, "
                     "torch.cuda.synchronize() around each call, device-resident tensors, one process; the profile: one "
                     "call per leg under the library's event profiler",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
