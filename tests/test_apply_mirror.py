"""CPU checks of tests/apply_mirror.c, the restatement the GPU apply tests compare against bit for bit: exact on
integer-valued inputs, within the standard bound of a chain of fused multiply-adds on random ones, NaN reaching exactly
the row / column it belongs to, and padding neither read nor written."""
import numpy as np
import pytest

from apply_cases import assert_same_bits, build_apply_mirror, minus_zero_member, mirror_apply, underflow_members

DTYPES = (np.float32, np.float64)
UNIT = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
SHAPES = [(1, 1), (1, 3), (5, 1), (8, 4), (17, 3), (64, 2), (100, 5), (128, 1)]


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return build_apply_mirror(tmp_path_factory.mktemp("apply_mirror"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_on_small_integers(dll, dtype):
    """|x|, |r| <= 15 and n <= 128: every partial sum is an integer below 2^15, exact in either format, so the chain
    equals the int64 product bit for bit."""
    rng = np.random.default_rng(11)
    for n, k in SHAPES:
        x = rng.integers(-15, 16, (n, n))
        r = rng.integers(-15, 16, (n, k))
        z = mirror_apply(dll, x.astype(dtype), r.astype(dtype))
        assert z.dtype == dtype and np.array_equal(z.astype(np.int64), x @ r), (n, k)
        assert not np.signbit(z[z == 0]).any()      # an exact zero of a chain that starts at +0 is +0


@pytest.mark.parametrize("dtype", DTYPES)
def test_within_the_fma_chain_bound(dll, dtype):
    """|z - x r| <= gamma_n sum_j |x_ij r_jk| with gamma_n = n u / (1 - n u): n roundings, one per fused multiply-add.
    The product that stands for the exact one is accumulated in the host's long double (64 significant bits where the
    platform has them), so that its own rounding does not eat into the bound of the float64 chain."""
    rng = np.random.default_rng(12)
    u = UNIT[dtype]
    for n, k in SHAPES:
        x = rng.uniform(-1, 1, (n, n)).astype(dtype)
        r = rng.uniform(-1, 1, (n, k)).astype(dtype)
        z = mirror_apply(dll, x, r)
        xl, rl = x.astype(np.longdouble), r.astype(np.longdouble)
        gamma = np.longdouble(n * u / (1 - n * u))
        bound = gamma * (np.abs(xl) @ np.abs(rl))
        assert (np.abs(z.astype(np.longdouble) - xl @ rl) <= bound).all(), (n, k)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_reaches_its_row_or_column_only(dll, dtype):
    rng = np.random.default_rng(13)
    n, k = 20, 4
    x = rng.uniform(-1, 1, (n, n)).astype(dtype)
    r = rng.uniform(-1, 1, (n, k)).astype(dtype)
    clean = mirror_apply(dll, x, r)
    xn = x.copy()
    xn[6, 11] = np.nan
    z = mirror_apply(dll, xn, r)
    assert np.isnan(z[6]).all() and not np.isnan(np.delete(z, 6, axis=0)).any()
    assert_same_bits(np.delete(z, 6, axis=0), np.delete(clean, 6, axis=0), "x")
    rn = r.copy()
    rn[9, 2] = np.nan
    z = mirror_apply(dll, x, rn)
    assert np.isnan(z[:, 2]).all() and not np.isnan(np.delete(z, 2, axis=1)).any()
    assert_same_bits(np.delete(z, 2, axis=1), np.delete(clean, 2, axis=1), "r")
    # a zero in x is multiplied through: 0 * inf is NaN
    xz, ri = x.copy(), r.copy()
    xz[3, 5] = 0.0
    ri[5, 1] = np.inf
    z = mirror_apply(dll, xz, ri)
    assert np.isnan(z[3, 1]) and np.isinf(np.delete(z[:, 1], 3)).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_padding_is_neither_read_nor_written(dll, dtype):
    rng = np.random.default_rng(14)
    n, k = 13, 3
    x = rng.uniform(-1, 1, (n, n)).astype(dtype)
    r = rng.uniform(-1, 1, (n, k)).astype(dtype)
    want = mirror_apply(dll, x, r)
    xp = np.full((n, n + 3), np.nan, dtype)
    rp = np.full((n, k + 2), np.nan, dtype)
    zp = np.full((n, k + 1), 7.5, dtype)
    xp[:, :n], rp[:, :k] = x, r
    mirror_apply(dll, xp[:, :n], rp[:, :k], out=zp[:, :k])
    assert_same_bits(zp[:, :k], want, "strided")
    assert (zp[:, k:] == 7.5).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_chain_can_end_in_minus_zero(dll, dtype):
    """A negative product below half the smallest subnormal rounds to -0 even onto +0, so -0 is a value a chain can
    hold and end in; and (+0)(+0) added to it would lose the sign, while (+0)(-0) keeps every value: the padding rule
    of the kernels."""
    x, r = minus_zero_member(dtype)
    z = mirror_apply(dll, x, r)
    assert (z == 0).all()
    assert np.signbit(z[0, 0]) and np.signbit(z[1, 0]) and not np.signbit(z[0, 1]) and not np.signbit(z[1, 1])
    # one more term with a +0 factor: beside -0 it changes no value the chain can hold, beside +0 it clears the sign
    for pad, kept in ((-0.0, True), (0.0, False)):
        more = np.add(np.multiply(dtype(0), dtype(pad), dtype=dtype), z, dtype=dtype)
        assert (np.signbit(more) == np.signbit(z)).all() == kept, pad
    for acc in (np.inf, -np.inf, 1.5, -1.5, np.finfo(dtype).smallest_subnormal):
        assert np.add(np.multiply(dtype(0), dtype(-0.0), dtype=dtype), dtype(acc), dtype=dtype) == dtype(acc)
    assert np.isnan(np.add(np.multiply(dtype(0), dtype(-0.0), dtype=dtype), dtype(np.nan), dtype=dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_underflow_members_reach_signed_zeros_and_subnormals(dll, dtype):
    """The inputs the GPU tests use for the signs of zeros do produce them."""
    xs, rs = underflow_members([3, 8, 5], 2, 150, dtype)
    z = np.concatenate([mirror_apply(dll, x, r) for x, r in zip(xs, rs)])
    zero = z == 0
    finfo = np.finfo(dtype)
    assert (zero & np.signbit(z)).any() and (zero & ~np.signbit(z)).any()
    assert ((np.abs(z) > 0) & (np.abs(z) < finfo.tiny)).any()
