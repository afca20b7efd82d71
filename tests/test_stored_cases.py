"""CPU checks of the NumPy restatement in tests/stored_cases.py against independent facts: the formats' rounding,
range and subnormal behaviour on hand-picked values, torch's own bfloat16 conversion, the double rounding through
float32, exact widening, the byte layout of a hand-worked batch and the statistics of hand-worked members."""
import numpy as np
import torch

import stored_cases as sc
from stored_cases import BFLOAT16, FLOAT16, FLOAT32, NATIVE

f32, f64 = np.float32, np.float64


def f16(x, dtype=f32):
    return float(sc.narrow(np.array([x], dtype), FLOAT16)[0])


def test_bfloat16_integer_form_is_torch_conversion():
    rng = np.random.default_rng(1)
    rand = rng.integers(0, 2 ** 32, 200_000, dtype=np.uint64).astype(np.uint32).view(f32)
    ties = (np.arange(0x3F80, 0x3FC0, dtype=np.uint32) << 16 | 0x8000).view(f32)          # exactly between two bfloat16
    near = np.concatenate([(ties.view(np.uint32) - 1).view(f32), (ties.view(np.uint32) + 1).view(f32)])
    edge = np.array([0.0, -0.0, np.inf, -np.inf, 2.0 ** -126, 2.0 ** -133, 2.0 ** -149, 3.4e38, -3.4e38, 3.3895314e38],
                    f32)
    x = np.concatenate([rand, ties, -ties, near, edge])
    x = x[~np.isnan(x)]
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(sc.bf16_bits(x), want)
    nan = sc.bf16_bits(np.array([np.nan, -np.nan], f32))
    assert np.isnan(sc.widen(nan, BFLOAT16, f32)).all()


def test_float16_ties_go_to_even_both_ways():
    assert f16(1 + 2.0 ** -11) == 1.0                      # down to the even neighbour
    assert f16(1 + 3 * 2.0 ** -11) == 1 + 2.0 ** -9        # up to the even neighbour
    assert f16(-(1 + 2.0 ** -11)) == -1.0


def test_float16_range_edges():
    assert f16(65504.0) == 65504.0
    assert f16(f32(65519.996)) == 65504.0
    assert f16(65520.0) == np.inf and f16(-65520.0) == -np.inf
    assert f16(np.inf) == np.inf and np.isnan(f16(np.nan))


def test_float16_subnormals():
    assert f16(2.0 ** -25) == 0.0 and not np.signbit(f16(2.0 ** -25))          # a tie: to the even neighbour, zero
    assert f16(np.nextafter(f32(2.0 ** -25), f32(1))) == 2.0 ** -24
    assert f16(2.0 ** -14) == 2.0 ** -14 and f16(2.0 ** -24) == 2.0 ** -24
    assert f16(3 * 2.0 ** -25) == 2.0 ** -23                                    # 1.5 units: a tie, up to the even 2
    z = sc.narrow(np.array([-(2.0 ** -25)], f32), FLOAT16)
    assert z[0] == 0 and np.signbit(z[0])                                       # a signed zero


def test_double_goes_through_float32():
    x = 1 + 2.0 ** -11 + 2.0 ** -30
    assert f16(x, f64) == 1.0                                                   # float32 drops 2^-30, then a tie
    with np.errstate(all="ignore"):
        assert float(np.array([x]).astype(np.float16)[0]) == 1 + 2.0 ** -10     # the direct conversion differs
    y = np.array([1 + 2.0 ** -8 + 2.0 ** -40], f64)                             # the same for bfloat16
    assert float(sc.roundtrip(y, BFLOAT16)[0]) == 1.0
    assert float(sc.narrow(np.array([1 + 2.0 ** -24 + 2.0 ** -50], f64), FLOAT32)[0]) == 1 + 2.0 ** -23


def test_widening_is_exact():
    h = np.arange(0, 1 << 16, dtype=np.uint16)
    half = h.view(np.float16)
    ok = ~np.isnan(half)
    for dtype in (f32, f64):
        w = sc.widen(half, FLOAT16, dtype)
        assert np.array_equal(w[ok].astype(np.float16).view(np.uint16), h[ok])
        assert np.array_equal(w[ok].astype(np.longdouble), half[ok].astype(np.longdouble))
        wb = sc.widen(h, BFLOAT16, dtype)
        okb = ~np.isnan(wb)
        assert np.array_equal(sc.bf16_bits(wb[okb].astype(f32)), h[okb])
        assert np.array_equal(wb.astype(f32).view(np.uint32)[okb], h.astype(np.uint32)[okb] << 16)
    s = np.array([2.0 ** -149, -(2.0 ** -126), 3.0e38, 1 + 2.0 ** -23], f32)
    assert np.array_equal(sc.widen(s, FLOAT32, f64).astype(f32).view(np.uint32), s.view(np.uint32))
    for code in (FLOAT16, BFLOAT16):                         # a value a format holds survives it
        x = sc.roundtrip(np.linspace(-3, 3, 1001).astype(f32), code)
        assert np.array_equal(sc.roundtrip(x, code), x)


def test_offsets_of_a_hand_worked_batch():
    # orders 3, 1, 2, 5 as float16, native, bfloat16, float32 of float64 members:
    # 18 bytes -> 24; 8 bytes -> 32; 8 bytes -> 40; 100 bytes -> 144
    off, size = sc.offsets([3, 1, 2, 5], [FLOAT16, NATIVE, BFLOAT16, FLOAT32], f64)
    assert off.tolist() == [0, 24, 32, 40] and size == 144
    # float32 members: native is 4 bytes.  orders 1, 1, 3: 2 -> 8; 4 -> 16; 36 -> 56
    off, size = sc.offsets([1, 1, 3], [FLOAT16, NATIVE, NATIVE], f32)
    assert off.tolist() == [0, 8, 16] and size == 56
    members = [np.array([[1.5]], f32), np.array([[-2.0]], f32), np.arange(9, dtype=f32).reshape(3, 3)]
    buf = sc.store_bytes(members, [FLOAT16, NATIVE, NATIVE])
    assert buf[:2].view(np.float16)[0] == 1.5 and (buf[2:8] == sc.FILL).all()
    assert buf[8:12].view(f32)[0] == -2.0 and (buf[12:16] == sc.FILL).all()
    assert np.array_equal(buf[16:52].view(f32), np.arange(9, dtype=f32)) and (buf[52:] == sc.FILL).all()
    gap = sc.gap_mask([1, 1, 3], [FLOAT16, NATIVE, NATIVE], f32)
    assert np.array_equal(gap, buf == sc.FILL) and gap.sum() == 6 + 4 + 4


def test_statistics_of_hand_worked_members():
    assert sc.block_stats(np.array([[1, -2], [-3, 0.5]], f32)) == (4.0, 3.0, 0.5)
    assert sc.block_stats(np.zeros((3, 3), f64)) == (0.0, 0.0, np.inf)
    assert sc.block_stats(np.array([[0, -0.0], [0, 2.0 ** -140]], f32)) == (2.0 ** -140, 2.0 ** -140, 2.0 ** -140)
    assert all(np.isnan(v) for v in sc.block_stats(np.array([[1, np.nan], [2, 3]], f32)))
    assert sc.block_stats(np.array([[1, -np.inf], [2, 3]], f64)) == (np.inf, np.inf, 1.0)
    # rows ascending, one addition each: 2^53 + 1 + 1 stays 2^53, 1 + 1 + 2^53 is 2^53 + 2
    assert sc.block_stats(np.array([[2.0 ** 53], [1], [1]], f64).repeat(3, 1))[0] == 2.0 ** 53
    assert sc.block_stats(np.array([[1], [1], [2.0 ** 53]], f64).repeat(3, 1))[0] == 2.0 ** 53 + 2


def test_special_values_hold_what_the_tests_pin():
    for dtype in (f32, f64):
        m = sc.special_values(dtype).reshape(-1)
        assert m.size == 64 and np.isnan(m).sum() == 1 and np.isinf(m).sum() == 2
        assert ((m == 0) & np.signbit(m)).sum() == 1 and ((m == 0) & ~np.signbit(m)).sum() == 1
        assert (m == dtype(1 + 2.0 ** -11)).any() and (m == dtype(2.0 ** -25)).any() and (m == 65520).any()
    assert (sc.special_values(f64) == 1 + 2.0 ** -11 + 2.0 ** -30).any()
