"""CPU proof of tests/tall_batch_cases.py, before the GPU sees any of it: the two transform identities hold bit for bit
on the oracle, and the library plans and routes the shapes of tests/test_gpu_tall_batches.py the way those tests need
-- asked through the C ABI with a null handle, the plan code needs no device.  No tolerance: bytes and literal plan values."""
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


ROUTE_KNOBS = ("MI32_PANEL_W", "MI32_BLOCK_W", "MI32_MULTI_PANEL", "MI32_ALGO", "MI32_LOOKAHEAD_MIN", "MI32_BATCH_SPLIT")
END, RIDE = 1, 0   # mi32_route_t.part_strips_at_end


def _route(n, batch):
    """(np, bw, blocks, shared, look-ahead, members per part, strips per part, first fused block) and the workgroups
    per panel by block, of mi32_resolve_route with a null handle."""
    r, groups = _lib.resolve_route(None, n, batch)
    assert r["parts"] in (1, 2) and len(groups) == r["nblocks"]
    assert r["part_batch"][r["parts"]:] == [0] * (2 - r["parts"]) and sum(r["part_batch"]) == batch
    return ((r["np"], r["block_width"], r["nblocks"], r["shared_panels"], r["lookahead"], r["part_batch"][:r["parts"]],
             r["part_strips_at_end"][:r["parts"]], r["first_fused_block"]), groups)


def test_every_route_above_4096_rows_is_reached_by_a_case(monkeypatch):
    """The routing table of DESIGN.md ("Routing above 4096 rows"), row by row, as the library itself routes the shapes
    of tests/test_gpu_tall_batches.py: asked of mi32_resolve_route, which answers from the one description the launcher
    runs a call from.  Literal values, no device."""
    for name in ROUTE_KNOBS:
        monkeypatch.delenv(name, raising=False)
    tall, wide = C.N_TALL, C.N_WIDE
    # batch 1: shared panels and the look-ahead, which moves the strips to the block's end.  Two workgroups per panel
    # in the first block only; blocks 9 ... 16 hold at most 2048 rows
    assert _route(tall, 1) == ((4224, 256, 17, 1, 1, [1], [END], 9), [2] + [1] * 16)
    # batch 2 ... 4: shared panels with a batch index, no look-ahead; strips ride for 2 and 3 (132 and 198 tiles), run
    # at the block's end for 4 (264) -- which is large enough to be split but keeps its shared panels, never split
    assert _route(tall, 2) == ((4224, 256, 17, 1, 0, [2], [RIDE], 9), [2] + [1] * 16)
    assert _route(tall, 3) == ((4224, 256, 17, 1, 0, [3], [RIDE], 9), [2] + [1] * 16)
    assert _route(tall, 4) == ((4224, 256, 17, 1, 0, [4], [END], 9), [2] + [1] * 16)
    # batch >= 5: one workgroup per panel (8 rows per lane: W = 8 in the first block), and the batch is split over two
    # streams; each half counts its own strip tiles
    assert _route(tall, 5) == ((4224, 256, 17, 0, 0, [3, 2], [RIDE, RIDE], 9), [1] * 17)
    assert _plan(tall, 5) == (16, 256, [8] + [16] * 16)
    assert _route(tall, 7) == ((4224, 256, 17, 0, 0, [4, 3], [END, RIDE], 9), [1] * 17)
    # batch >= 8 and 64 Mi elements: block width 128
    assert _route(tall, 8) == ((4224, 128, 33, 0, 0, [4, 4], [END, END], 17), [1] * 33)
    assert _plan(tall, 7)[1] == 256 and _plan(tall, 8)[1] == 128
    # three workgroups per panel, going 3 -> 2 -> 1 (8320, 8192 and 4096 rows are the edges): 3 in block 0 only, 2 up
    # to block 16 (4224 rows), 1 from block 17 (3968 rows) on
    groups_wide = [3] + [2] * 16 + [1] * 16
    assert _route(wide, 1) == ((8320, 256, 33, 1, 1, [1], [END], 25), groups_wide)
    assert _route(wide, 2) == ((8320, 256, 33, 1, 0, [2], [END], 25), groups_wide)       # 260 tiles
    assert [groups_wide[b] for b in (0, 1, 16, 17)] == [3, 2, 2, 1]
    assert -(-(8320 - 128) // 4096) == 2 and -(-(8320 - 240) // 4096) == 2   # 3 -> 2 inside the FIRST block
    assert all(set(_plan(n, b)[2]) == {16} for n, b in ((tall, 1), (tall, 2), (tall, 3), (tall, 4), (wide, 1), (wide, 2)))
    # above 8192 rows without shared panels: 16 rows per lane, W = 4
    assert _route(wide, 5) == ((8320, 256, 33, 0, 0, [3, 2], [END, END], 25), [1] * 33)
    five = _plan(wide, 5)
    assert five == (16, 256, [4] + [8] * 16 + [16] * 16)
    # up to 4096 rows: no shared panels, no look-ahead, the strips ride; four matrices are 2^26 elements and split
    assert _route(4096, 1) == ((4096, 256, 16, 0, 0, [1], [RIDE], 8), [1] * 16)
    assert _route(4096, 4) == ((4096, 256, 16, 0, 0, [2, 2], [RIDE, RIDE], 8), [1] * 16)   # 128 tiles each
    # MI32_BATCH_SPLIT=0: one part, which counts all 330 tiles
    monkeypatch.setenv("MI32_BATCH_SPLIT", "0")
    assert _route(tall, 5) == ((4224, 256, 17, 0, 0, [5], [END], 9), [1] * 17)
    monkeypatch.delenv("MI32_BATCH_SPLIT")
    # MI32_MULTI_PANEL=0: the single matrix that stands in for a batch of five plans the same widths and keeps its
    # look-ahead
    monkeypatch.setenv("MI32_MULTI_PANEL", "0")
    assert _route(wide, 1) == ((8320, 256, 33, 0, 1, [1], [END], 25), [1] * 33)
    assert _plan(wide, 1) == five
    assert _plan(tall, 1)[2] == _plan(tall, 5)[2] == [8] + [16] * 16


def test_each_routing_threshold_has_a_shape_on_either_side(monkeypatch):
    """One (n, batch) on each side of every threshold of plan_route, at the smallest shape that has the edge."""
    for name in ROUTE_KNOBS:
        monkeypatch.delenv(name, raising=False)
    route = lambda n, batch: _lib.resolve_route(None, n, batch)[0]   # noqa: E731
    # fused blocks: at most 2048 rows
    assert route(2048, 1)["first_fused_block"] == 0
    assert (route(2176, 1)["np"], route(2176, 1)["first_fused_block"], route(2176, 1)["nblocks"]) == (2176, 1, 9)
    # shared panels and the look-ahead: more than 4096 padded rows; shared panels up to four matrices
    lo, hi = route(4096, 1), route(4224, 1)
    assert (lo["np"], lo["shared_panels"], lo["lookahead"]) == (4096, 0, 0)
    assert (hi["np"], hi["shared_panels"], hi["lookahead"]) == (4224, 1, 1)
    assert route(4224, 4)["shared_panels"] == 1 and route(4224, 5)["shared_panels"] == 0
    # strips: they ride up to 256 tiles of 64 columns (128 rows: two per member)
    assert (route(128, 128)["parts"], route(128, 128)["part_strips_at_end"]) == (1, [0, 0])
    assert (route(128, 129)["parts"], route(128, 129)["part_strips_at_end"]) == (1, [1, 0])
    # split: from four matrices and 2^26 elements on
    assert (route(4096, 4)["parts"], route(4096, 4)["part_batch"]) == (2, [2, 2])
    assert (route(4095, 4)["parts"], route(4095, 4)["part_batch"]) == (1, [4, 0])
    assert route(4096, 3)["parts"] == 1
    # block width 128: from eight matrices and 2^26 elements on (8 x 2896^2 < 2^26 <= 8 x 2897^2)
    assert 8 * 2896 ** 2 < 2 ** 26 <= 8 * 2897 ** 2
    assert route(2896, 8)["block_width"] == 256 and route(2897, 8)["block_width"] == 128
    assert route(4200, 7)["block_width"] == 256
    # MI32_LOOKAHEAD_MIN: the fewest padded rows with the look-ahead; values up to 2048 mean 2048
    assert route(2300, 1)["lookahead"] == 0
    for value in ("2048", "100"):
        monkeypatch.setenv("MI32_LOOKAHEAD_MIN", value)
        assert (route(2300, 1)["np"], route(2300, 1)["lookahead"]) == (2304, 1)
        assert route(2300, 1)["part_strips_at_end"] == [1, 0]
        assert route(2048, 1)["lookahead"] == 1 and route(1920, 1)["lookahead"] == 0
    # what the blocked path does not take
    lib = _lib.load()
    r = _lib.Route()
    for n, batch in ((0, 1), (4200, 0), (16385, 1)):
        assert lib.mi32_resolve_route(None, n, batch, ctypes.byref(r), None, 0) == _lib.MI32_BAD_SHAPE
    assert lib.mi32_resolve_route(None, 16384, 1, ctypes.byref(r), None, 0) == _lib.MI32_OK and r.np == 16384
