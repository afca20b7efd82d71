"""Inputs and helpers of the register-resident path's tests (tests/test_gpu_resident.py, tests/test_resident_abi.py).
The matrix families are those of tests/test_gpu_parity.py, restated here so that the two files stay independent."""
import numpy as np

from conftest import gate_matrix

FP64_ORDERS = [1, 2, 3, 5, 8, 9, 16, 17, 31, 32, 33, 48, 63, 64]
TIE_ORDERS = [8, 12, 16, 24, 32, 48, 64]
BIG_BATCHES = [(8, 70_000), (5, 66_000)]
# the three shapes whose direction tests/test_gpu_resident.py asserts, and the parent's workspace for each
TIMED_SHAPES = [(8, 16_384), (32, 4_096), (64, 2_048)]


def dist_matrix(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "gate":
        return gate_matrix(n, seed)
    if kind == "ref100":  # U(0, 100)
        return rng.uniform(0, 100, (n, n)).astype(np.float32)
    if kind == "rand":    # U(0, 1)
        return rng.uniform(0, 1, (n, n)).astype(np.float32)
    if kind == "hollow":  # U(0, 100) with a zero diagonal: every step must swap
        a = rng.uniform(0, 100, (n, n))
        np.fill_diagonal(a, 0.0)
        return a.astype(np.float32)
    raise ValueError(kind)


def dominant(n, seed, dtype):
    """Strictly diagonally dominant: what the no-pivot variant is for."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, (n, n))
    a[np.arange(n), np.arange(n)] = np.abs(a).sum(axis=1) + 1.0
    return a.astype(dtype)


def tie_batch(n, members=16):
    """Small-integer matrices drawn in sequence from one generator: many equal magnitudes per column, so the
    lowest-row-among-equals rule decides pivots."""
    rng = np.random.default_rng(31_000 + n)
    return np.stack([rng.integers(-4, 5, (n, n)).astype(np.float32) for _ in range(members)])


def big_batch(n, batch):
    """`batch` well-conditioned, row-permuted matrices from ONE generator."""
    rng = np.random.default_rng(4100 + n)
    a = rng.uniform(-1, 1, (batch, n, n)) + np.sqrt(n) * np.eye(n)
    perm = rng.permuted(np.tile(np.arange(n), (batch, 1)), axis=1)
    return np.take_along_axis(a, perm[:, :, None], axis=1).astype(np.float32)


def shared_wave_batch():
    """9 matrices of order 20 (two per wave at 32 lanes each): member 3 rank 1, member 5 with a NaN, member 8 zero."""
    mats = np.stack([gate_matrix(20, 600 + b) for b in range(9)])
    mats[3] = 1.0
    mats[5, 4, 7] = np.nan
    mats[8] = 0.0
    return mats, [0, 0, 0, 2, 0, 2, 0, 0, 2]


def run(inv, a):
    """Invert a numpy matrix or batch (its dtype is kept) on the device; (inverse, status) as numpy arrays."""
    import torch

    ta = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    x, st = inv.inv(ta)
    torch.cuda.synchronize()
    return x.cpu().numpy(), st.cpu().numpy()


def oracle_batch(fn, mats, n):
    """(inverses (B, n, n), statuses) of the CPU oracle function `fn(vec, n, return_info=True)` over a batch."""
    out = np.empty_like(mats)
    st = np.empty(len(mats), np.int64)
    for b, m in enumerate(mats):
        x, info = fn(m, n, return_info=True)
        out[b] = x.reshape(n, n)
        st[b] = info["status"]
    return out, st
