"""GPU self-test of v_fmac_f32_dpp / v_cndmask_b32_dpp with row_newbcast (one wave-uniform row of 16 floats in one
register): both forms against __builtin_fmaf and a plain select computed in the same launch, word for word, on
denormals, signed zeros, infinities and products that need the single rounding.  The panel step does not use the
forms (they issue slower than a plain FMA: DESIGN.md section 4, round 4); the test keeps what is known about the
hardware checked."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gpu_matrix_inversion_amd import _lib  # noqa: E402

SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x80800000,
                     0x7f800000, 0xff800000, 0x7f7fffff, 0xff7fffff, 0x3f800000, 0xbf800000, 0x3f800001, 0x3f7fffff,
                     0x33800000, 0x34000000, 0x4b800000, 0x3effffff], dtype=np.uint32)


def _selftest_inputs(ncases, seed):
    rng = np.random.default_rng(seed)
    w = np.empty((ncases, 3, 64), dtype=np.uint32)
    for c in range(ncases):
        kind = c % 4
        if kind == 0:    # special values in every operand
            w[c] = rng.choice(SPECIALS, (3, 64))
        elif kind == 1:  # any finite or infinite bit pattern (no NaN operand: its payload's way through is not at issue)
            bits = rng.integers(0, 1 << 32, (3, 64), dtype=np.uint64).astype(np.uint32)
            nan = ((bits & 0x7f800000) == 0x7f800000) & ((bits & 0x007fffff) != 0)
            w[c] = np.where(nan, bits & np.uint32(0xff800000), bits)
        elif kind == 2:  # (1 + i ulp)(1 + j ulp) - 1: the product's low bits survive only with a single rounding
            row = (1.0 + rng.integers(1, 1 << 12, 64) * 2.0 ** -23).astype(np.float32)
            f = (1.0 + rng.integers(1, 1 << 12, 64) * 2.0 ** -23).astype(np.float32)
            acc = np.full(64, 1.0, dtype=np.float32)  # dst = fma(row, -f, 1.0)
            w[c] = np.stack([row, f, acc]).view(np.uint32)
        else:            # denormal products and sums
            row = rng.uniform(-1, 1, 64).astype(np.float32) * np.float32(2.0 ** -70)
            f = rng.uniform(-1, 1, 64).astype(np.float32) * np.float32(2.0 ** -65)
            acc = rng.integers(0, 1 << 10, 64).astype(np.uint32).view(np.float32)
            w[c] = np.stack([row, f, acc]).view(np.uint32)
    return w


def test_dpp_row_forms_match_builtin_fmaf_word_for_word():
    ncases = 64
    w = _selftest_inputs(ncases, 5)
    d_in = torch.from_numpy(w.view(np.int32)).cuda()
    d_out = torch.zeros((ncases, 16, 4, 64), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    lib = _lib.load()
    assert lib.mi32_debug_dpp_selftest(ctypes.c_void_p(d_in.data_ptr()), ctypes.c_void_p(d_out.data_ptr()), ncases,
                                       None) == 0
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint32)
    # the reference words themselves, recomputed here where float64 holds the result exactly: entry C of each row of 16
    row = w[:, 0].view(np.float32).reshape(ncases, 4, 16)
    lanes = np.arange(64)
    for c in range(16):
        rc = np.repeat(row[:, :, c], 16, axis=1)
        pick = (np.arange(ncases) * 7 + 5 * c) & 63
        want_sel = np.where(lanes[None, :] == pick[:, None], rc, w[:, 2].view(np.float32)).view(np.uint32)
        assert np.array_equal(out[:, c, 3], want_sel), c
    bad_f = np.argwhere(out[:, :, 0] != out[:, :, 1])
    bad_s = np.argwhere(out[:, :, 2] != out[:, :, 3])
    print("row_fmac mismatches", len(bad_f), "row_select mismatches", len(bad_s))
    assert len(bad_f) == 0, [(tuple(i), hex(out[i[0], i[1], 0, i[2]]), hex(out[i[0], i[1], 1, i[2]])) for i in bad_f[:8]]
    assert len(bad_s) == 0, [(tuple(i), hex(out[i[0], i[1], 2, i[2]]), hex(out[i[0], i[1], 3, i[2]])) for i in bad_s[:8]]
    # the test must have met what it is for: results that a separately rounded product would get wrong
    k2 = np.arange(ncases) % 4 == 2
    got = out[k2][:, 0, 0].view(np.float32).astype(np.float64)
    r0 = np.repeat(row[k2][:, :, 0], 16, axis=1).astype(np.float64)
    f = w[k2, 1].view(np.float32).astype(np.float64)
    assert np.array_equal(got, (1.0 - r0 * f).astype(np.float32).astype(np.float64))  # exact in float64
    two_roundings = (np.float32(1.0) - (r0 * f).astype(np.float32)).astype(np.float64)
    assert (got != two_roundings).any()
