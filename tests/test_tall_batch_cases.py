"""CPU proof of tests/tall_batch_cases.py, before the GPU sees any of it: the two transform identities hold bit for bit
on the oracle, and the library plans the shapes of tests/test_gpu_tall_batches.py the way those tests need -- asked
through the C ABI with a null handle, the plan code needs no device.  No tolerance: bytes and literal plan values."""
import ctypes

import numpy as np
import pytest

import tall_batch_cases as C
from conftest import canonical_bytes

from gpu_matrix_inversion_amd import _lib

ORDERS = [130, 300]   # 2 and 44 above a multiple of 128


@pytest.mark.parametrize("kind", ["gate", "ref100"])
@pytest.mark.parametrize("n", ORDERS)
def test_row_permuted_sign_flipped_scaled_variant_has_the_transformed_inverse_bit_for_bit(oracle, kind, n):
    a = C.base_member(kind, n, 7 + n)
    forms = {"inplace": oracle.matrix_inv_32_inplace,
             "blocked_exact": lambda m, order, **kw: oracle.matrix_inv_32_blocked_exact(m, order, 128, **kw)}
    for form, fn in forms.items():
        x, info = fn(a, n, return_info=True)
        assert info["status"] == 0
        for k in sorted(set(C.VARIANT_KS)):
            a1, t = C.variant(a, 50 + k, k)
            assert not np.array_equal(t.perm, np.arange(n)) and {-1.0, 1.0} == set(t.d.tolist())
            x1, info1 = fn(a1, n, return_info=True)
            assert info1["status"] == 0
            assert canonical_bytes(x1) == canonical_bytes(C.apply_variant(x, t)), (kind, n, form, k)
            # the same rows win, in the places the permutation put them
            assert np.array_equal(t.perm[_rows_in_input(info1["pivots"])], _rows_in_input(info["pivots"])), (form, k)


def _rows_in_input(pivots):
    """Which row of the INPUT each step took: ``pivots[j]`` is a position at step j, after the earlier swaps."""
    n = pivots.size
    at = np.arange(n)
    out = np.empty(n, np.int64)
    for j in range(n):
        p = int(pivots[j])
        out[j] = at[p]
        at[p], at[j] = at[j], at[p]
    return out


def test_variants_of_one_base_differ_and_the_transform_is_not_the_identity(oracle):
    """apply_variant on a wrong transform must not pass: two variants of one base have different expected inverses, and
    neither is the base's."""
    n = 130
    a = C.base_member("gate", n, 1)
    x = oracle.matrix_inv_32_inplace(a, n)
    (a1, t1), (a2, t2) = C.variant(a, 1, 3), C.variant(a, 2, 3)
    assert not np.array_equal(a1, a2)
    e1, e2 = C.apply_variant(x, t1), C.apply_variant(x, t2)
    assert canonical_bytes(e1) != canonical_bytes(e2) != canonical_bytes(x)
    assert canonical_bytes(oracle.matrix_inv_32_inplace(a2, n)) == canonical_bytes(e2)


@pytest.mark.parametrize("n", ORDERS)
def test_diagonally_scaled_variant_has_the_scaled_inverse_without_pivoting_bit_for_bit(oracle, n):
    a = C.dominant(n, 500 + n)
    x, info = oracle.matrix_inversion_no_pivots(a, n, return_info=True)
    assert x.dtype == np.float32 and info["status"] == 0
    a1, t = C.variant_nopivot(a, 9)
    for d in (t.d1, t.d2):
        m, e = np.frexp(np.abs(d))
        assert (m == 0.5).all() and e.min() >= -7 and e.max() <= 9 and {-1.0, 1.0} == set(np.sign(d).tolist())
    x1, info1 = oracle.matrix_inversion_no_pivots(a1, n, return_info=True)
    assert info1["status"] == 0
    assert canonical_bytes(x1) == canonical_bytes(C.apply_variant_nopivot(x, t))
    assert canonical_bytes(x1) != canonical_bytes(x)


def test_batches_hold_two_independent_bases_and_one_full_division_member(oracle):
    for batch in (2, 3, 4, 5, 8):
        ms = C.tall_batch(300, batch)
        assert len(ms) == batch and [m.transform for m in ms[:2]] == [None, None]
        assert [m.base[0] for m in ms] == ["gate", "ref100"] * (batch // 2) + ["gate"] * (batch % 2)
        ks = [m.transform.k for m in ms[2:]]
        assert ks.count(C.K_FULL_DIVISION) == (1 if batch > 2 else 0)
        perms = [m.transform.perm.tobytes() for m in ms[2:]]
        assert len(set(perms)) == len(perms)
        for m in ms:
            assert m.matrix.dtype == np.float32 and m.matrix.shape == (300, 300)
    rot = C.tall_batch(300, 2, rotate=1)
    assert rot[0].transform is None and rot[0].base[0] == "ref100"
    assert rot[1].base[0] == "gate" and rot[1].transform.k == C.K_FULL_DIVISION
    # every member's expected inverse is the oracle's own result on that member (n = 300: cheap enough to run all)
    for m in C.tall_batch(300, 8):
        got, info = oracle.matrix_inv_32_inplace(m.matrix, 300, return_info=True)
        assert info["status"] == 0
        assert canonical_bytes(got) == canonical_bytes(C.expected_inverse(oracle, m))
    # the full-division member really leaves the fast division's range [2^-47, 2^48): its inverse is 2^-40 x the
    # base's, most of it below 2^-47 (one numerator out of range puts the whole strip on the full division)
    big = C.tall_batch(300, 3)[2]
    med_big, med_base = (float(np.median(np.abs(C.expected_inverse(oracle, m)))) for m in (big, ms[0]))
    assert 0 < med_big == med_base * 2.0 ** -40 < 2.0 ** -47 < med_base


def _plan(n, batch):
    lib = _lib.load()
    w, bw, nb = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    buf = (ctypes.c_int * 128)()
    assert lib.mi32_resolve_blocking(None, n, batch, ctypes.byref(w), ctypes.byref(bw)) == _lib.MI32_OK
    assert lib.mi32_resolve_panel_widths(None, n, batch, buf, 128, ctypes.byref(nb)) == _lib.MI32_OK
    return w.value, bw.value, [int(buf[i]) for i in range(nb.value)]


@pytest.mark.parametrize("n,batch,multi,bw,widths", C.PLANS,
                         ids=[f"{n}x{b}" + ("" if m is None else f"-multi{m}") for n, b, m, _, _ in C.PLANS])
def test_plans_the_gpu_tests_rely_on(monkeypatch, n, batch, multi, bw, widths):
    """Asked with a null handle (AUTO, no blocking set): what a fresh Inverter gets.  The environment is read per call."""
    for name in ("MI32_PANEL_W", "MI32_BLOCK_W", "MI32_MULTI_PANEL", "MI32_ALGO"):
        monkeypatch.delenv(name, raising=False)
    if multi is not None:
        monkeypatch.setenv("MI32_MULTI_PANEL", multi)
    assert _lib.load().mi32_resolve_algo(None, n, batch) == _lib.ALGO_BLOCKED
    w, got_bw, got = _plan(n, batch)
    assert (w, got_bw) == (16, bw)
    assert got == widths and len(got) == -(-(-(-n // 128) * 128) // bw)


def test_every_route_above_4096_rows_is_reached_by_a_case(monkeypatch):
    """The routing table of DESIGN.md ("Routing above 4096 rows"), row by row, as the thresholds in the code give it
    for the shapes of tests/test_gpu_tall_batches.py."""
    for name in ("MI32_PANEL_W", "MI32_BLOCK_W", "MI32_MULTI_PANEL", "MI32_ALGO"):
        monkeypatch.delenv(name, raising=False)
    tall, wide = C.N_TALL, C.N_WIDE
    shared = lambda n, b: set(_plan(n, b)[2]) == {16}   # noqa: E731  (all-16 above 4096 rows: shared panels are on)
    # batch 2 ... 4: shared panels with a batch index; strips ride for 2 and 3, run at the block's end for 4
    assert all(shared(tall, b) for b in (1, 2, 3, 4)) and not shared(tall, 5)
    assert [C.strips_ride_in_panel_launches(tall, b) for b in (2, 3, 4)] == [True, True, False]
    assert C.shared_panel_groups(tall, 256, 0) == 2 and C.shared_panel_groups(tall, 256, 1) == 1
    # three workgroups per panel, going 3 -> 2 -> 1 inside the FIRST block (8320, 8192 and 4096 rows are the edges)
    assert shared(wide, 2) and not C.strips_ride_in_panel_launches(wide, 2)
    assert C.shared_panel_groups(wide, 256, 0) == 3 and -(-(8320 - 128) // 4096) == 2 and -(-(8320 - 240) // 4096) == 2
    assert [C.shared_panel_groups(wide, 256, b) for b in (1, 16, 17)] == [2, 2, 1]
    # batch >= 5: one workgroup per panel, and the batch is split over two streams; a batch of 4 is large enough to
    # be split but keeps its shared panels, which are never split
    assert [C.would_split(tall, b) for b in (2, 3, 4, 5, 8)] == [False, False, True, True, True]
    assert _plan(tall, 5)[2][0] == 8 and _plan(tall, 5)[1] == 256
    # batch >= 8 and 64 Mi elements: block width 128
    assert _plan(tall, 7)[1] == 256 and _plan(tall, 8)[1] == 128
    # above 8192 rows without shared panels: 16 rows per lane, W = 4 -- a batch of 5 and the single matrix with
    # MI32_MULTI_PANEL=0 that stands in for it plan the same widths
    five = _plan(wide, 5)
    monkeypatch.setenv("MI32_MULTI_PANEL", "0")
    assert _plan(wide, 1) == five and five[2][0] == 4
    assert _plan(tall, 1)[2] == _plan(tall, 5)[2] == [8] + [16] * 16
