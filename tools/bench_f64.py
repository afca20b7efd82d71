#!/usr/bin/env python3
"""Diagnostic: fp64 inversion time (matrix_inversion_FP64 of the reference), sweep vs blocked, per block width.

    python tools/bench_f64.py [N ...]                          pivoting, a row-permuted gate matrix
    python tools/bench_f64.py --no-pivot [--batch B] [N ...]   matrix_inversion_no_pivots on a diagonally dominant
                                                               matrix; --batch also times B such matrices in one call
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gpu_matrix_inversion_amd as g  # noqa: E402


def gate(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, (n, n)) + np.sqrt(n) * np.eye(n)
    return a[rng.permutation(n)]


def dominant(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, (n, n))
    return a + np.diag(np.abs(a).sum(axis=1) + 1.0)


def time_inv(inv, a, reps):
    x, st = inv.inv(a)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        inv.inv(a, out=x)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, x, st


def main():
    args = sys.argv[1:]
    nopivot = "--no-pivot" in args
    batch = 0
    if "--batch" in args:
        batch = int(args[args.index("--batch") + 1])
        del args[args.index("--batch"):args.index("--batch") + 2]
    sizes = [int(v) for v in args if not v.startswith("--")] or [1024, 2048, 4096, 8192]
    legs = [("sweep", dict(algo="sweep")), ("blocked bw64", dict(algo="auto", block_width=64)),
            ("blocked bw128", dict(algo="auto", block_width=128))]
    if not nopivot:
        legs.append(("blocked bw256", dict(algo="auto", block_width=256)))
    for n in sizes:
        a = torch.from_numpy(dominant(n, n) if nopivot else gate(n, n)).cuda()
        eye = torch.eye(n, dtype=torch.float64, device="cuda")
        for label, kw in legs:
            if label == "sweep" and n > 4096:
                continue
            inv = g.Inverter(pivoting=not nopivot, **kw)
            dt, x, st = time_inv(inv, a, 3 if n >= 4096 else 5)
            res = float((a @ x - eye).abs().sum(dim=1).max())
            inv.set_profiling(True)
            inv.get_profile()
            inv.inv(a, out=x)
            prof = {k: (round(v[0], 2), v[1]) for k, v in inv.get_profile().items() if v[1]}
            print(f"N={n:5d} {label:14s} {1e3 * dt:9.2f} ms  {2.0 * n ** 3 / dt / 1e12:6.2f} TFLOP/s  residual {res:.2e}  status {int(st[0])}  {prof}")
            inv.close()
        if batch:
            ab = torch.stack([torch.from_numpy(dominant(n, n + b) if nopivot else gate(n, n + b)) for b in range(batch)]).cuda()
            inv = g.Inverter(algo="auto", pivoting=not nopivot)
            dt, x, st = time_inv(inv, ab, 3)
            res = max(float((ab[b] @ x[b] - eye).abs().sum(dim=1).max()) for b in range(batch))
            print(f"N={n:5d} batch {batch:3d} auto bw{inv.resolved_blocking_f64(n):<4d} {1e3 * dt:9.2f} ms  "
                  f"{2.0 * batch * n ** 3 / dt / 1e12:6.2f} TFLOP/s  max residual {res:.2e}  status {st.tolist()}")
            inv.close()


if __name__ == "__main__":
    main()
