"""NumPy restatements and inputs of the stored-inverse tests (tests/test_stored_cases.py, tests/test_stored_args.py,
tests/test_gpu_stored.py): narrowing and widening of the four storage formats, the store's byte layout, the block
statistics and the choice of a format, all as include/mat_inv_32_stored.h defines them, plus the input families.

Format codes: 0 native (the working type), 1 float32 (float64 members only), 2 float16, 3 bfloat16."""
import numpy as np

NATIVE, FLOAT32, FLOAT16, BFLOAT16 = 0, 1, 2, 3
# code: (unit roundoff, smallest normal, largest finite)
LIMITS = {FLOAT32: (2.0 ** -24, 2.0 ** -126, (2.0 - 2.0 ** -23) * 2.0 ** 127),
          FLOAT16: (2.0 ** -11, 2.0 ** -14, 65504.0),
          BFLOAT16: (2.0 ** -8, 2.0 ** -126, (2.0 - 2.0 ** -7) * 2.0 ** 127)}
FILL = 0xA5


def codes_of(dtype):
    """The codes a member of `dtype` takes."""
    return (NATIVE, FLOAT32, FLOAT16, BFLOAT16) if np.dtype(dtype) == np.float64 else (NATIVE, FLOAT16, BFLOAT16)


def elem_bytes(code, dtype):
    return {NATIVE: np.dtype(dtype).itemsize, FLOAT32: 4, FLOAT16: 2, BFLOAT16: 2}[code]


def bf16_bits(f32):
    """bfloat16 bits of float32 values: the integer form, round-to-nearest-even; a NaN stays a NaN."""
    u = np.ascontiguousarray(f32, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(f32)
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


def narrow(x, code):
    """`x` (float32 or float64) in storage format `code`, as an array of the stored element type (uint16 bits for
    bfloat16): round-to-nearest-even, IEEE results, float64 to a 16-bit format through float32."""
    x = np.asarray(x)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if code == NATIVE:
            return x.copy()
        if code == FLOAT32:
            assert x.dtype == np.float64
            return x.astype(np.float32)
        f32 = x.astype(np.float32)
        return f32.astype(np.float16) if code == FLOAT16 else bf16_bits(f32)


def widen(stored, code, dtype):
    """The stored elements back in `dtype`: exact."""
    if code == BFLOAT16:
        stored = (np.asarray(stored, np.uint16).astype(np.uint32) << 16).view(np.float32)
    with np.errstate(invalid="ignore"):          # (a signalling NaN is quieted: no news)
        return np.asarray(stored).astype(dtype)


def roundtrip(x, code):
    """widen(narrow(x)): what the apply kernel multiplies by."""
    return widen(narrow(x, code), code, x.dtype)


def offsets(orders, formats, dtype):
    """(byte offset of every member, size of the store): off_0 = 0, off_{b+1} = round_up_8(off_b + n_b^2 bytes(F_b))."""
    off, at = [], 0
    for n, f in zip(orders, formats):
        off.append(at)
        at = (at + int(n) * int(n) * elem_bytes(int(f), dtype) + 7) // 8 * 8
    return np.array(off, np.int64), at


def store_bytes(members, formats, fill=FILL):
    """The store as a uint8 array: every member narrowed, row-major and dense at its offset; the bytes between members
    keep `fill`."""
    dtype = members[0].dtype
    off, size = offsets([m.shape[0] for m in members], formats, dtype)
    buf = np.full(size, fill, np.uint8)
    for m, f, o in zip(members, formats, off):
        raw = np.ascontiguousarray(narrow(m, int(f))).reshape(-1).view(np.uint8)
        buf[o:o + raw.size] = raw
    return buf


def gap_mask(orders, formats, dtype):
    """True at the bytes of the store that belong to no member."""
    off, size = offsets(orders, formats, dtype)
    gap = np.ones(size, bool)
    for n, f, o in zip(orders, formats, off):
        gap[o:o + int(n) * int(n) * elem_bytes(int(f), dtype)] = False
    return gap


def block_stats(a):
    """(norm1, absmax, absmin) of one member in float64: column sums from +0 over the rows ascending, one addition per
    row (an explicit loop: np.sum adds pairwise); absmin over the nonzero entries, +inf without any; three NaNs if any
    entry is a NaN."""
    a = np.asarray(a)
    if np.isnan(a).any():
        return (np.nan, np.nan, np.nan)
    mag = np.abs(a.astype(np.float64))
    c = np.zeros(a.shape[1], np.float64)
    with np.errstate(over="ignore"):
        for i in range(a.shape[0]):
            c = c + mag[i]
    nz = mag[mag != 0]
    return (float(c.max()), float(mag.max()), float(nz.min()) if nz.size else np.inf)


def stats_of(members):
    return np.array([block_stats(m) for m in members], np.float64).reshape(len(members), 3)


def choose(dtype, kappa, absmax, absmin, tol=0.1, status=None):
    """The format of every member, member by member in Python floats (which are float64): the first of float16,
    bfloat16, float32 (float64 members only) with kappa finite, kappa * u <= tol, absmax <= largest finite and absmin
    >= smallest normal; native otherwise and where status != 0."""
    order = (FLOAT16, BFLOAT16, FLOAT32) if np.dtype(dtype) == np.float64 else (FLOAT16, BFLOAT16)
    out = np.zeros(len(kappa), np.int32)
    for b in range(len(kappa)):
        if (status is not None and int(status[b]) != 0) or not np.isfinite(kappa[b]):
            continue
        for code in order:
            u, small, large = LIMITS[code]
            if float(kappa[b]) * u <= tol and float(absmax[b]) <= large and float(absmin[b]) >= small:
                out[b] = code
                break
    return out


# ---- inputs ----
def cycling_formats(orders, dtype, shift=0):
    """Formats cycling through the codes of `dtype` in ORDER-sorted position, so that every lane class that holds at
    least as many members as there are codes holds every format, and neighbours in a wave differ."""
    codes = codes_of(dtype)
    out = np.zeros(len(orders), np.int32)
    for rank, b in enumerate(np.argsort(np.asarray(orders), kind="stable")):
        out[b] = codes[(rank + shift) % len(codes)]
    return out


def members_in_range(orders, seed, dtype):
    """Members with entries +-2^U(-12, 12): inside float16's normal range, so that every format keeps them finite and
    normal, and roundings differ between the formats."""
    rng = np.random.default_rng(seed)
    out = []
    for n in orders:
        n = int(n)
        out.append((rng.choice([-1.0, 1.0], (n, n)) * 2.0 ** rng.uniform(-12, 12, (n, n))).astype(dtype))
    return out


def special_values(dtype):
    """An order-8 member (64 entries) of the values the narrowing tests pin, beside +-0, +-inf and a NaN; the rest are
    ordinary values.  The float64 form adds the double-rounding example, which float32 cannot hold."""
    f32 = np.float32
    vals = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65504.0, float(f32(65519.996)), 65520.0, 2.0 ** -25,
            float(np.nextafter(f32(2.0 ** -25), f32(1))), 2.0 ** -14, 2.0 ** -24, 3 * 2.0 ** -25, 0.0, -0.0, np.inf, -np.inf,
            np.nan, -(1 + 2.0 ** -11), -65520.0, -(2.0 ** -25), 2.0 ** -126, 2.0 ** -130, 2.0 ** 127, 3.0e38, 1 + 2.0 ** -8,
            1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, 2.0 ** -149]
    if np.dtype(dtype) == np.float64:
        vals += [1 + 2.0 ** -11 + 2.0 ** -30, 1 + 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -50, 1e300, -1e-300, 2.0 ** -1074]
    rng = np.random.default_rng(77)
    m = rng.uniform(-2, 2, 64)
    m[:len(vals)] = vals
    return m.astype(dtype).reshape(8, 8)
