"""GPU tests of the workgroup-resident path (``Inverter(algo="workgroup")``, ``MI32_ALGO=4``; run with ``-m gpu`` on
an MI355X): orders 65 ... 128, fp32 and fp64, with partial pivoting and without.

There is no tolerance anywhere in this file: the path does the sweep's arithmetic element by element, so every
member whose oracle status is 0 must equal the step-by-step CPU oracle bit for bit (``np.array_equal``), and every
status word must equal the oracle's.
"""
import ctypes

import numpy as np
import pytest

from batch_helpers import assert_members_equal, median_ms
from conftest import gate_matrix
from workgroup_cases import (BIG_BATCH, BIG_DISTINCT, BIG_ORDER, FP64_ORDERS, KINDS, MEMBERS, ORDERS, SLOT_ORDERS,
                             TIE_ORDERS, TIMED_SHAPES, big_distinct, big_index, dominant, dominant_batch, family_batch,
                             mixed_batch, oracle_batch, run, slot_batch_of_three, tie_batch, zero_diagonal_entry)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_matrix_inversion_amd as g  # noqa: E402


@pytest.fixture(scope="module")
def inv_wg():
    inv = g.Inverter(algo="workgroup")
    yield inv
    inv.close()


@pytest.fixture(scope="module")
def inv_wg_nopivot():
    inv = g.Inverter(algo="workgroup", pivoting=False)
    yield inv
    inv.close()


@pytest.mark.parametrize("n", ORDERS)
def test_fp32_every_order_bit_identical_to_oracle(oracle, inv_wg, n):
    assert inv_wg.resolved_algo(n, MEMBERS) == g.ALGO_WORKGROUP == 4
    assert inv_wg.resolved_workgroup(n)[0] == 256
    for kind in KINDS:
        mats = family_batch(kind, n)
        want, want_st = oracle_batch(oracle.matrix_inv_32, mats, n)
        got, st = run(inv_wg, mats)
        assert list(want_st) == [0] * MEMBERS and list(st) == [0] * MEMBERS, (kind, n, list(st), list(want_st))
        assert_members_equal(got, want, (kind, n))


@pytest.mark.parametrize("n", FP64_ORDERS)
def test_fp64_bit_identical_to_oracle(oracle, inv_wg, n):
    for kind in KINDS:
        mats = family_batch(kind, n).astype(np.float64)
        want, want_st = oracle_batch(oracle.matrix_inv_64, mats, n)
        got, st = run(inv_wg, mats)
        assert got.dtype == np.float64
        assert list(want_st) == [0] * MEMBERS and list(st) == [0] * MEMBERS, (kind, n, list(st), list(want_st))
        assert_members_equal(got, want, (kind, n))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("n", FP64_ORDERS)
def test_no_pivot_bit_identical_to_oracle(oracle, inv_wg_nopivot, n, dtype):
    assert inv_wg_nopivot.resolved_algo(n, MEMBERS) == g.ALGO_WORKGROUP
    mats = dominant_batch(n, dtype)
    want, want_st = oracle_batch(oracle.matrix_inversion_no_pivots, mats, n)
    got, st = run(inv_wg_nopivot, mats)
    assert got.dtype == dtype
    assert list(want_st) == [0] * MEMBERS and list(st) == [0] * MEMBERS
    assert_members_equal(got, want, (n, dtype))
    h = zero_diagonal_entry(n, dtype)
    want_h = oracle.matrix_inversion_no_pivots(h, n, return_info=True)[1]["status"]
    _, st = run(inv_wg_nopivot, h)
    assert int(st[0]) == want_h == oracle.STATUS_SINGULAR


@pytest.mark.parametrize("n", TIE_ORDERS)
def test_ties_the_lowest_row_wins(oracle, inv_wg, n):
    mats = tie_batch(n)
    assert mats.shape == (16, n, n)
    want, want_st = oracle_batch(oracle.matrix_inv_32, mats, n)
    assert list(want_st) == [0] * 16   # no member is skipped: a singular draw fails here
    got, st = run(inv_wg, mats)
    assert list(st) == [0] * 16
    assert_members_equal(got, want, n)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("n", SLOT_ORDERS)
def test_the_pivot_in_every_slab_and_slot(oracle, inv_wg, n, dtype):
    """Member 1 is the anti-diagonal permutation: the pivot of step r sits in register slot n - 1 - r, so every case of
    the pick / put switch of both slabs and both label registers is visited.  Member 0 is a signed power-of-two
    permutation; both inverses are exact and known in closed form, and the oracle agrees with them.  Member 2 is a
    dense matrix.  The wide path's test of this name (tests/test_gpu_wide.py) runs the same loops of the same body."""
    mats, exact = slot_batch_of_three(n, dtype)
    assert mats.shape == (3, n, n) and mats.dtype == dtype
    want, want_st = oracle_batch(oracle.matrix_inv_32 if dtype == np.float32 else oracle.matrix_inv_64, mats, n)
    assert list(want_st) == [0, 0, 0] and np.array_equal(want[:2], exact)
    got, st = run(inv_wg, mats)
    assert got.dtype == dtype and list(st) == [0, 0, 0]
    assert_members_equal(got, want, (n, dtype))


def test_invalid_members_among_valid_ones(oracle, inv_wg):
    """Members 2 (rank 1), 4 (a NaN) and 6 (all zero) are invalid; their neighbours must not notice."""
    mats, want_st = mixed_batch()
    n = mats.shape[1]
    want, oracle_st = oracle_batch(oracle.matrix_inv_32, mats, n)
    assert list(oracle_st) == want_st
    got, st = run(inv_wg, mats)
    assert list(st) == want_st
    for b in range(len(mats)):
        if want_st[b] == 0:
            assert np.array_equal(got[b], want[b]), b


def test_more_members_than_a_grid_dimension_holds(oracle, inv_wg):
    """Above 65535 members the sweep and blocked paths cannot be launched (the batch index is a grid y / z
    coordinate).  The batch indexes 256 distinct oracle-checked matrices in a shuffled order; every member is
    compared, none sampled."""
    assert BIG_BATCH > 65_535
    distinct = big_distinct()
    want, want_st = oracle_batch(oracle.matrix_inv_32, distinct, BIG_ORDER)
    assert want_st.shape == (BIG_DISTINCT,) and not want_st.any()
    idx = big_index()
    assert idx.shape == (BIG_BATCH,) and set(idx.tolist()) == set(range(BIG_DISTINCT))
    ta = torch.from_numpy(distinct).cuda()[torch.from_numpy(idx).cuda()].contiguous()
    assert ta.shape == (BIG_BATCH, BIG_ORDER, BIG_ORDER)
    x, st = inv_wg.inv(ta)
    torch.cuda.synchronize()
    assert not st.any().item(), torch.nonzero(st)[:8]
    tw = torch.from_numpy(want).cuda()[torch.from_numpy(idx).cuda()]
    diff = torch.nonzero((x != tw).flatten(1).any(dim=1)).flatten()
    assert diff.numel() == 0 and torch.equal(x, tw), diff[:8]


def test_host_entry_points_select_it_through_the_environment(oracle, monkeypatch):
    monkeypatch.setenv("MI32_ALGO", "4")
    a = gate_matrix(100, 81)
    assert np.array_equal(g.matrix_inv_32(a.reshape(-1), 100), oracle.matrix_inv_32(a, 100))
    mats = np.stack([gate_matrix(72, 8100 + b) for b in range(300)])
    out, st = g.matrix_inv_32_batched(mats)
    want, want_st = oracle_batch(oracle.matrix_inv_32, mats, 72)
    assert not st.any() and not want_st.any() and np.array_equal(out, want)
    a64 = gate_matrix(97, 82).astype(np.float64)
    assert np.array_equal(g.matrix_inv_64(a64.reshape(-1), 97), oracle.matrix_inv_64(a64, 97))
    d64 = dominant(128, 628, np.float64)
    assert np.array_equal(g.matrix_inversion_no_pivots(d64.reshape(-1), 128), oracle.matrix_inversion_no_pivots(d64, 128))
    b113 = gate_matrix(113, 83)
    got, times = g.fp32_bench(b113.reshape(-1), 113)
    assert np.array_equal(got, oracle.matrix_inv_32(b113, 113))
    assert times["pivot"] > 0 and times["column"] == 0 and times["makeAug"] == 0, times
    # an invalid matrix is the empty array, as on the other paths
    assert g.matrix_inv_32(np.ones(100 * 100, np.float32), 100).size == 0
    assert g.matrix_inv_64(np.ones(97 * 97), 97).size == 0


def test_small_orders_resolve_to_the_resident_path(inv_wg):
    n = 40
    assert inv_wg.resolved_algo(n, 9) == g.ALGO_RESIDENT
    assert inv_wg.resolved_workgroup(n) == (0, 0, 128)
    mats = np.stack([gate_matrix(n, 8300 + b) for b in range(9)])
    res = g.Inverter(algo="resident")
    try:
        want, want_st = run(res, mats)
    finally:
        res.close()
    got, st = run(inv_wg, mats)
    assert not st.any() and not want_st.any() and np.array_equal(got, want)


@pytest.mark.parametrize("n", [129, 200])
def test_larger_orders_fall_back_to_what_auto_resolves_to(inv_wg, n):
    a = gate_matrix(n, 8400 + n)
    auto = g.Inverter(algo="auto")
    try:
        assert inv_wg.resolved_algo(n, 1) == auto.resolved_algo(n, 1) != g.ALGO_WORKGROUP
        want, want_st = run(auto, a)
    finally:
        auto.close()
    assert inv_wg.resolved_workgroup(n) == (0, 0, 128)
    got, st = run(inv_wg, a)
    assert st[0] == want_st[0] == 0
    assert np.array_equal(got, want)


def test_asynchronous_pure_and_deterministic(inv_wg):
    n, batch = 90, 500
    a = torch.from_numpy(np.stack([gate_matrix(n, 8600 + b) for b in range(batch)])).cuda()
    keep = a.clone()
    x0, st0 = inv_wg.inv(a)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    out = torch.empty_like(a)
    with torch.cuda.stream(s):
        x1, st1 = inv_wg.inv(a, out=out)
    s.synchronize()
    torch.cuda.synchronize()
    assert x1.data_ptr() == out.data_ptr()
    assert torch.equal(a, keep)                       # the input is not modified
    assert torch.equal(x0, x1) and not st0.any() and not st1.any()
    # the look-ahead switch changes nothing for this path
    inv_wg.set_lookahead(False)
    try:
        x2, _ = inv_wg.inv(a)
        torch.cuda.synchronize()
    finally:
        inv_wg.set_lookahead(True)
    assert torch.equal(x0, x2)
    # d_status = NULL is allowed by the C ABI: the context keeps the status words itself
    out2 = torch.empty_like(a)
    inv_wg._bind_stream()
    rc = inv_wg._lib.mi32_inv_device(inv_wg._h, ctypes.c_void_p(a.data_ptr()), n, batch,
                                     ctypes.c_void_p(out2.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(out2, x0)
    a64 = a[:100].double()
    w64, _ = inv_wg.inv(a64)
    out64 = torch.empty_like(a64)
    rc = inv_wg._lib.mi32_inv_device_f64(inv_wg._h, ctypes.c_void_p(a64.data_ptr()), n, 100,
                                         ctypes.c_void_p(out64.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(out64, w64)


@pytest.mark.parametrize("n,batch", TIMED_SHAPES)
def test_faster_than_the_path_auto_resolves_to(inv_wg, n, batch):
    """Only the direction is asserted (no ratio was known before this path existed): for these two batches one
    workgroup-resident launch must beat what AUTO does today, the blocked path, which this change does not touch
    and which therefore stands in for the parent commit.  Both are timed in this one process, medians of 5 calls
    after 2 warm-ups, AUTO with its workspace reserved first.  n = 128 is deliberately not asserted; the ratios
    measured on an MI355X are in DESIGN.md and profiles/workgroup/medium_batch.json."""
    rng = np.random.default_rng(9800 + n)
    mats = rng.uniform(-1, 1, (batch, n, n)) + np.sqrt(n) * np.eye(n)
    a = torch.from_numpy(mats.astype(np.float32)).cuda()
    out = torch.empty_like(a)
    st = torch.empty(batch, dtype=torch.int32, device=a.device)
    auto = g.Inverter(algo="auto")
    try:
        assert auto.resolved_algo(n, batch) == g.ALGO_BLOCKED
        auto.reserve(n, batch)
        t_auto = median_ms(lambda: auto.inv(a, out=out, status=st))
        x_auto = out.clone()
        assert not st.any()
    finally:
        auto.close()
    assert inv_wg.resolved_algo(n, batch) == g.ALGO_WORKGROUP
    t_wg = median_ms(lambda: inv_wg.inv(a, out=out, status=st))
    assert not st.any()
    print(f"\nn={n} batch={batch}: workgroup {t_wg:.3f} ms, auto {t_auto:.3f} ms, ratio {t_auto / t_wg:.2f}x")
    assert torch.equal(out, x_auto)      # both evaluate the reference's operation order
    assert t_wg < t_auto, (n, batch, t_wg, t_auto)
