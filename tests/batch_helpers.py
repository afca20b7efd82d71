"""Helpers shared by the GPU tests of the one-launch batch paths (no pytest in here: the test files import what they
need)."""
import statistics
import time

import numpy as np


def median_ms(fn, warmup=2, calls=5):
    """Median wall-clock milliseconds of `calls` synchronised calls of fn() after `warmup` untimed ones."""
    import torch

    ts = []
    for i in range(warmup + calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def assert_members_equal(got, want, tag):
    """Every member of `got` equals its member of `want` bit for bit, in number, dtype and value."""
    assert len(got) == len(want)
    for b in range(len(want)):
        assert got[b].dtype == want[b].dtype and np.array_equal(got[b], want[b]), \
            (tag, b, want[b].shape, float(np.abs(got[b] - want[b]).max()))


def strided(mats, pad, fill):
    """The members one after the other at leading dimension n + pad; the padding columns hold `fill`.  Returns
    (flat buffer, element offset per member, leading dimensions, padding mask)."""
    lds = np.array([m.shape[0] + pad for m in mats], np.int32)
    sizes = np.array([m.shape[0] * ld for m, ld in zip(mats, lds)], np.int64)
    off = np.concatenate(([0], np.cumsum(sizes)[:-1]))
    buf = np.full(int(sizes.sum()), fill, mats[0].dtype)
    is_pad = np.ones(buf.size, bool)
    for m, o, ld in zip(mats, off, lds):
        n = m.shape[0]
        buf[o:o + n * ld].reshape(n, ld)[:, :n] = m
        is_pad[o:o + n * ld].reshape(n, ld)[:, :n] = False
    return buf, off, lds, is_pad
