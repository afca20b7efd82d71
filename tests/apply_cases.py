"""Inputs and helpers of the apply tests (tests/test_apply_mirror.py, tests/test_apply_abi.py, tests/test_gpu_apply.py):
the restatement of Z = X R as one chain of fused multiply-adds per component (tests/apply_mirror.c), the bit comparison
the GPU tests use, and the launch rule of include/mat_inv_32_c.h restated."""
import ctypes
import os
import subprocess

import numpy as np

LANE_TOPS = (8, 16, 32, 64, 128)   # the largest order each of the five lane classes takes; its lanes per member


def build_apply_mirror(directory):
    """Compile tests/apply_mirror.c into `directory` with the host C compiler, in the oracle's way (no contraction:
    every fused multiply-add is spelled out), and load it."""
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "apply_mirror.c")
    lib = os.path.join(str(directory), "libapply_mirror.so")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                           "-o", lib, src, "-lm"])
    dll = ctypes.CDLL(lib)
    for fn in (dll.apply_mirror_f32, dll.apply_mirror_f64):
        fn.restype = None
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                       ctypes.c_void_p, ctypes.c_int]
    return dll


def _last_stride(t):
    assert t.ndim == 2 and t.strides[1] == t.itemsize and t.strides[0] % t.itemsize == 0
    return t.strides[0] // t.itemsize


def mirror_apply(dll, x, r, out=None):
    """Z of one float32 / float64 member: x is (n, n), r is (n, k) of x's dtype; both may be views with a row stride
    (the padding behind a row is then neither read nor written).  `out`: an (n, k) view to write into."""
    assert x.ndim == 2 and x.shape[0] == x.shape[1] and x.dtype in (np.float32, np.float64)
    assert r.ndim == 2 and r.shape[0] == x.shape[0] and r.shape[1] >= 1 and r.dtype == x.dtype
    z = np.empty(r.shape, r.dtype) if out is None else out
    assert z.shape == r.shape and z.dtype == r.dtype
    fn = dll.apply_mirror_f32 if x.dtype == np.float32 else dll.apply_mirror_f64
    fn(x.ctypes.data, x.shape[0], _last_stride(x), r.ctypes.data, r.shape[1], _last_stride(r), z.ctypes.data,
       _last_stride(z))
    return z


def mirror_apply_members(dll, xs, rs):
    """The members' Z one below the other: the packed right-hand-side layout."""
    return np.concatenate([mirror_apply(dll, x, r) for x, r in zip(xs, rs)])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_same_bits(got, want, tag):
    """NaN exactly where `want` has one (payloads are not compared), the same bits everywhere else, signs of zeros
    included."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (tag, "NaN pattern", int(np.isnan(got).sum()), int(nan.sum()))
    bad = (bits(got) != bits(want)) & ~nan
    assert not bad.any(), (tag, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def rows_of(zs, orders):
    """The members' row ranges of a packed right-hand side."""
    off = np.concatenate(([0], np.cumsum(np.asarray(orders, np.int64))))
    return [zs[off[b]:off[b + 1]] for b in range(len(orders))]


def rhs_members(orders, k, seed, dtype=np.float32):
    """One (n, k) right-hand side per member, U(-1, 1), drawn in member order from one generator."""
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1.0, 1.0, (int(n), k)).astype(dtype) for n in orders]


def tiny(dtype):
    """A magnitude whose square lies below half the smallest subnormal of `dtype`: a product of two such values rounds
    to a zero of the product's sign."""
    return dtype(2.0 ** -80) if dtype == np.float32 else dtype(2.0 ** -540)


def minus_zero_member(dtype):
    """(x, r) of order 3, two columns, whose chains END in a signed zero: the last term of rows 0 and 1 is a negative
    product that underflows, so z[0] and z[1] are -0 in column 0 (+0 in column 1, whose last product is positive);
    row 2 passes through -0 and ends on a term with an exact zero factor."""
    t = tiny(dtype)
    x = np.array([[0, 0, -t], [0, -t, -t], [0, -t, 0]], dtype)
    r = np.array([[1, 1], [t, t], [t, -t]], dtype)
    return x, r


def underflow_members(orders, k, seed, dtype):
    """(xs, rs) whose chains pass through and end in subnormals and zeros of both signs.  Entries are +-U(0.5, 1) times
    a scale: `tiny`, or `sub`, whose square is subnormal.  R: the first n // 2 rows at `sub`, the rest at `tiny`.  X: the
    last n - n // 2 columns at `tiny`, so that every chain's tail is made of products that underflow; the first n // 2
    columns by row: exact zeros (every product of the row underflows: the result is a zero with the sign of the last
    term), `sub` (a subnormal result), or `sub` and 1 mixed (a normal one)."""
    rng = np.random.default_rng(seed)
    sub = dtype(2.0 ** -70) if dtype == np.float32 else dtype(2.0 ** -530)

    def draw(shape, scales):
        v = rng.uniform(0.5, 1.0, shape) * rng.choice([-1.0, 1.0], shape)
        return v.astype(dtype) * np.asarray(scales, dtype)[rng.integers(0, len(scales), shape)]

    xs, rs = [], []
    for n in (int(n) for n in orders):
        h = n // 2
        head = draw((n, h), [1.0, sub])
        head[0::3] = 0
        head[1::3] = draw(head[1::3].shape, [sub])
        xs.append(np.ascontiguousarray(np.concatenate([head, draw((n, n - h), [tiny(dtype)])], axis=1), dtype))
        rs.append(np.concatenate([draw((h, k), [sub]), draw((n - h, k), [tiny(dtype)])]).astype(dtype))
    return xs, rs


def lanes_of(n):
    """Lanes per member: the smallest of 8 / 16 / 32 / 64 / 128 that is at least the order."""
    return next(top for top in LANE_TOPS if n <= top)


def chunk_cols(elem_bytes):
    """The columns a group holds at a time: 32 bytes of accumulators per lane."""
    return 32 // elem_bytes


def expected_launches(orders, nrhs, elem_bytes=4):
    """[(first, count, lanes, chunk_cols)] of mi32_vbatch_apply_launches: one launch per lane class that has members,
    over the member list sorted by order, whatever nrhs is."""
    srt = sorted(int(n) for n in orders)
    out = []
    for top in LANE_TOPS:
        idx = [i for i, n in enumerate(srt) if lanes_of(n) == top]
        if idx:
            out.append((idx[0], len(idx), top, chunk_cols(elem_bytes)))
    return out
