"""GPU tests of the register-resident path (``Inverter(algo="resident")``, ``MI32_ALGO=3``; run with ``-m gpu`` on
an MI355X): orders 1 ... 64, fp32 and fp64, with partial pivoting and without.

There is no tolerance anywhere in this file: the path does the sweep's arithmetic element by element, so every
member whose oracle status is 0 must equal the step-by-step CPU oracle bit for bit (``np.array_equal``), and every
status word must equal the oracle's.
"""
import ctypes

import numpy as np
import pytest

from batch_helpers import assert_members_equal, median_ms
from conftest import gate_matrix
from resident_cases import (BIG_BATCHES, FP64_ORDERS, TIE_ORDERS, TIMED_SHAPES, big_batch, dist_matrix, dominant,
                            oracle_batch, run, shared_wave_batch, tie_batch)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_matrix_inversion_amd as g  # noqa: E402
from gpu_matrix_inversion_amd import _lib  # noqa: E402

KINDS = ("gate", "ref100", "rand", "hollow")


@pytest.fixture(scope="module")
def inv_res():
    inv = g.Inverter(algo="resident")
    yield inv
    inv.close()


@pytest.fixture(scope="module")
def inv_res_nopivot():
    inv = g.Inverter(algo="resident", pivoting=False)
    yield inv
    inv.close()


def _batch_of_7(kind, n):
    # 7 is odd on purpose: with fewer than 64 lanes per matrix the last wave is partly empty
    return np.stack([dist_matrix(kind, n, 9000 + 100 * n + b) for b in range(7)])


@pytest.mark.parametrize("n", range(1, 65))
def test_fp32_every_order_bit_identical_to_oracle(oracle, inv_res, n):
    assert inv_res.resolved_algo(n, 7) == g.ALGO_RESIDENT
    for kind in KINDS:
        if kind == "hollow" and n == 1:
            continue
        mats = _batch_of_7(kind, n)
        want, want_st = oracle_batch(oracle.matrix_inv_32, mats, n)
        got, st = run(inv_res, mats)
        assert list(want_st) == [0] * 7 and list(st) == [0] * 7, (kind, n, list(st), list(want_st))
        assert_members_equal(got, want, (kind, n))


@pytest.mark.parametrize("n", FP64_ORDERS)
def test_fp64_bit_identical_to_oracle(oracle, inv_res, n):
    for kind in KINDS:
        if kind == "hollow" and n == 1:
            continue
        mats = _batch_of_7(kind, n).astype(np.float64)
        want, want_st = oracle_batch(oracle.matrix_inv_64, mats, n)
        got, st = run(inv_res, mats)
        assert got.dtype == np.float64
        assert list(want_st) == [0] * 7 and list(st) == [0] * 7, (kind, n, list(st), list(want_st))
        assert_members_equal(got, want, (kind, n))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("n", FP64_ORDERS)
def test_no_pivot_bit_identical_to_oracle(oracle, inv_res_nopivot, n, dtype):
    assert inv_res_nopivot.resolved_algo(n, 5) == g.ALGO_RESIDENT
    mats = np.stack([dominant(n, 500 + n + b, dtype) for b in range(5)])
    want, want_st = oracle_batch(oracle.matrix_inversion_no_pivots, mats, n)
    got, st = run(inv_res_nopivot, mats)
    assert got.dtype == dtype
    assert list(want_st) == [0] * 5 and list(st) == [0] * 5
    assert_members_equal(got, want, (n, dtype))
    if n >= 3:
        h = mats[0].copy()
        h[1, 1] = 0.0
        h[1, 0] = 0.0        # keeps the (1,1) entry exactly zero after step 0
        want_h = oracle.matrix_inversion_no_pivots(h, n, return_info=True)[1]["status"]
        _, st = run(inv_res_nopivot, h)
        assert int(st[0]) == want_h == oracle.STATUS_SINGULAR


@pytest.mark.parametrize("n", TIE_ORDERS)
def test_ties_the_lowest_row_wins(oracle, inv_res, n):
    mats = tie_batch(n)
    assert mats.shape == (16, n, n)
    want, want_st = oracle_batch(oracle.matrix_inv_32, mats, n)
    assert list(want_st) == [0] * 16   # no member is skipped: a singular draw fails here
    got, st = run(inv_res, mats)
    assert list(st) == [0] * 16
    assert_members_equal(got, want, n)


def test_status_inside_a_shared_wave(oracle, inv_res):
    """Members 3 and 5 are invalid and share a wave (32 lanes per matrix of order 20) with valid ones."""
    mats, want_st = shared_wave_batch()
    assert inv_res.resolved_resident(20) == (32, 64)
    want, oracle_st = oracle_batch(oracle.matrix_inv_32, mats, 20)
    assert list(oracle_st) == want_st
    got, st = run(inv_res, mats)
    assert list(st) == want_st
    for b in range(9):
        if want_st[b] == 0:
            assert np.array_equal(got[b], want[b]), b


@pytest.mark.parametrize("n,batch", BIG_BATCHES)
def test_more_members_than_a_grid_dimension_holds(oracle, inv_res, n, batch):
    """Above 65535 members the sweep and blocked paths cannot be launched (the batch index is a grid y / z
    coordinate).  Every member is compared, none sampled."""
    assert batch > 65_535
    mats = big_batch(n, batch)
    want, want_st = oracle_batch(oracle.matrix_inv_32, mats, n)
    assert not want_st.any()
    got, st = run(inv_res, mats)
    assert not st.any(), np.nonzero(st)[0][:8]
    diff = np.nonzero((got != want).any(axis=(1, 2)))[0]
    assert diff.size == 0 and np.array_equal(got, want), diff[:8]


def test_host_entry_points_select_it_through_the_environment(oracle, monkeypatch):
    monkeypatch.setenv("MI32_ALGO", "3")
    a = gate_matrix(40, 71)
    assert np.array_equal(g.matrix_inv_32(a.reshape(-1), 40), oracle.matrix_inv_32(a, 40))
    mats = np.stack([gate_matrix(12, 7100 + b) for b in range(300)])
    out, st = g.matrix_inv_32_batched(mats)
    want, want_st = oracle_batch(oracle.matrix_inv_32, mats, 12)
    assert not st.any() and not want_st.any() and np.array_equal(out, want)
    a64 = gate_matrix(33, 72).astype(np.float64)
    assert np.array_equal(g.matrix_inv_64(a64.reshape(-1), 33), oracle.matrix_inv_64(a64, 33))
    d64 = dominant(64, 564, np.float64)
    assert np.array_equal(g.matrix_inversion_no_pivots(d64.reshape(-1), 64), oracle.matrix_inversion_no_pivots(d64, 64))
    b50 = gate_matrix(50, 73)
    got, times = g.fp32_bench(b50.reshape(-1), 50)
    assert np.array_equal(got, oracle.matrix_inv_32(b50, 50))
    assert times["pivot"] > 0 and times["column"] == 0 and times["makeAug"] == 0, times
    # an invalid matrix is the empty array, as on the other paths
    assert g.matrix_inv_32(np.ones(40 * 40, np.float32), 40).size == 0
    assert g.matrix_inv_64(np.ones(33 * 33), 33).size == 0


@pytest.mark.parametrize("n", [65, 200])
def test_larger_orders_fall_back_to_what_auto_resolves_to(oracle, inv_res, n):
    auto = g.Inverter(algo="auto")
    try:
        assert inv_res.resolved_algo(n, 1) == auto.resolved_algo(n, 1) != g.ALGO_RESIDENT
    finally:
        auto.close()
    assert inv_res.resolved_resident(n) == (0, 64)
    a = gate_matrix(n, 7400 + n)
    want, info = oracle.matrix_inv_32_inplace(a, n, return_info=True)
    got, st = run(inv_res, a)
    assert st[0] == info["status"] == 0
    assert np.array_equal(got.reshape(-1), want)


def test_asynchronous_pure_and_deterministic(inv_res):
    n, batch = 24, 1000
    a = torch.from_numpy(np.stack([gate_matrix(n, 7600 + b) for b in range(batch)])).cuda()
    keep = a.clone()
    x0, st0 = inv_res.inv(a)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    out = torch.empty_like(a)
    with torch.cuda.stream(s):
        x1, st1 = inv_res.inv(a, out=out)
    s.synchronize()
    torch.cuda.synchronize()
    assert x1.data_ptr() == out.data_ptr()
    assert torch.equal(a, keep)                       # the input is not modified
    assert torch.equal(x0, x1) and not st0.any() and not st1.any()
    # the look-ahead switch changes nothing for this path
    inv_res.set_lookahead(False)
    try:
        x2, _ = inv_res.inv(a)
        torch.cuda.synchronize()
    finally:
        inv_res.set_lookahead(True)
    assert torch.equal(x0, x2)
    # d_status = NULL is allowed by the C ABI: the context keeps the status words itself
    out2 = torch.empty_like(a)
    inv_res._bind_stream()
    rc = inv_res._lib.mi32_inv_device(inv_res._h, ctypes.c_void_p(a.data_ptr()), n, batch,
                                      ctypes.c_void_p(out2.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(out2, x0)
    a64 = a[:100].double()
    w64, _ = inv_res.inv(a64)
    out64 = torch.empty_like(a64)
    rc = inv_res._lib.mi32_inv_device_f64(inv_res._h, ctypes.c_void_p(a64.data_ptr()), n, 100,
                                          ctypes.c_void_p(out64.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(out64, w64)


ONE_BODY_ORDERS = (3, 4, 8, 13, 16, 20, 32)
ONE_BODY_BATCH = 37   # a multiple of no groups-per-workgroup count (4 ... 32): the last workgroup holds empty groups


@pytest.mark.parametrize("pivoting", [True, False], ids=["pivot", "nopivot"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_one_body_every_kernel_family_gives_the_same_bits(oracle, inv_res, inv_res_nopivot, dtype, pivoting):
    """The kernels of mi32_resident.hip share one load, one step loop and one store: the inverse, the inverse beside
    the determinant and A X = I must agree bit for bit, uniform and variable-size alike.  With K = n identity columns
    the uniform solve runs at widths 6, 8, 16, 26, 32, 40 and 64: every lane class, both edges of a class, and a width
    whose class is not the order's.  The variable-size calls take all seven orders interleaved in one plan, so groups
    of different order share waves.  No tolerance; every status word must be 0.  The anchor against the CPU oracle
    (order 13) keeps kernels that are all wrong alike from passing."""
    inv = inv_res if pivoting else inv_res_nopivot
    tdtype = torch.float32 if dtype == np.float32 else torch.float64
    rng = np.random.default_rng(9100)
    mats = {}
    for n in ONE_BODY_ORDERS:
        a = rng.uniform(-1, 1, (ONE_BODY_BATCH, n, n)) + n * np.eye(n)   # diagonally dominant: non-singular
        if pivoting:
            a = np.stack([m[rng.permutation(n)] for m in a])
        mats[n] = a.astype(dtype)
    kmax = max(ONE_BODY_ORDERS)
    uniform = {}
    for n in ONE_BODY_ORDERS:
        a = torch.from_numpy(mats[n]).cuda()
        x, st = inv.inv(a)
        xd, std, mant, exp = inv.inv_det(a)
        xs, sts = inv.solve(a, torch.eye(n, dtype=tdtype, device="cuda").repeat(ONE_BODY_BATCH, 1, 1))
        assert not st.any() and not std.any() and not sts.any(), n
        assert torch.equal(xd, x), n
        assert torch.equal(xs, x), n
        uniform[n] = (x.cpu(), mant.cpu(), exp.cpu())
    # the anchor
    fn = (oracle.matrix_inv_32 if dtype == np.float32 else oracle.matrix_inv_64) if pivoting \
        else oracle.matrix_inversion_no_pivots
    want, want_st = oracle_batch(fn, mats[13], 13)
    assert not want_st.any()
    assert_members_equal(uniform[13][0].numpy(), want, 13)
    # one plan: [3, 32, 4, 20, 8, 16, 13] repeated, member b of order n is mats[n][b]
    pattern = (3, 32, 4, 20, 8, 16, 13)
    orders = np.tile(pattern, ONE_BODY_BATCH)
    members = [mats[n][b] for b in range(ONE_BODY_BATCH) for n in pattern]
    a_flat = torch.from_numpy(np.concatenate([m.reshape(-1) for m in members])).cuda()
    # B: every member's identity, padded with zero columns to the widest order
    rhs = torch.from_numpy(np.concatenate([np.eye(m.shape[0], kmax, dtype=dtype) for m in members])).cuda()
    plan = inv.plan_ragged(orders)
    try:
        xr, str_ = inv.inv_ragged(plan, a_flat)
        xrd, strd, (rmant, rexp) = inv.inv_ragged(plan, a_flat, det=True)
        xrs, strs = inv.solve_ragged(plan, a_flat, rhs)
        # the same B four columns wide: widths 7 ... 36, so that orders 3 / 4 and 13 / 16 / 20 share the waves of one
        # solve launch and a finished group sits out the steps of its neighbours
        xrn, strn = inv.solve_ragged(plan, a_flat, rhs[:, :4].contiguous())
        torch.cuda.synchronize()
    finally:
        plan.close()
    assert not str_.any() and not strd.any() and not strs.any() and not strn.any()
    assert torch.equal(xrd, xr)
    xr, xrs, xrn, rmant, rexp = xr.cpu(), xrs.cpu(), xrn.cpu(), rmant.cpu(), rexp.cpu()
    at = row = 0
    for i, n in enumerate(orders):
        b = i // len(pattern)
        x, mant, exp = uniform[n]
        assert torch.equal(xr[at:at + n * n].view(n, n), x[b]), (i, n)
        assert torch.equal(xrs[row:row + n, :n], x[b]), (i, n)
        assert not xrs[row:row + n, n:].any(), (i, n)          # A X = 0 has the solution 0
        k = min(n, 4)
        assert torch.equal(xrn[row:row + n, :k], x[b][:, :k]), (i, n)
        assert rmant[i] == mant[b] and rexp[i] == exp[b], (i, n)
        at += n * n
        row += n


@pytest.mark.parametrize("n,batch", TIMED_SHAPES)
def test_faster_than_the_path_auto_resolves_to(inv_res, n, batch):
    """Only the direction is asserted (no ratio was known before this path existed): for these three batches of
    small matrices one resident launch must beat what AUTO does today -- the sweep path below 32 rows, the blocked
    path from 32 on -- timed in the same process, medians of 5 calls after 2 warm-ups.  The ratios measured on an
    MI355X are in DESIGN.md and profiles/resident/small_batch.json."""
    rng = np.random.default_rng(8800 + n)
    mats = rng.uniform(-1, 1, (batch, n, n)) + np.sqrt(n) * np.eye(n)
    a = torch.from_numpy(mats.astype(np.float32)).cuda()
    out = torch.empty_like(a)
    st = torch.empty(batch, dtype=torch.int32, device=a.device)
    auto = g.Inverter(algo="auto")
    try:
        assert auto.resolved_algo(n, batch) == (g.ALGO_SWEEP if n < 32 else g.ALGO_BLOCKED)
        auto.reserve(n, batch)
        t_auto = median_ms(lambda: auto.inv(a, out=out, status=st))
        x_auto = out.clone()
        assert not st.any()
    finally:
        auto.close()
    t_res = median_ms(lambda: inv_res.inv(a, out=out, status=st))
    assert not st.any()
    print(f"\nn={n} batch={batch}: resident {t_res:.3f} ms, auto {t_auto:.3f} ms, ratio {t_auto / t_res:.1f}x")
    assert torch.equal(out, x_auto)      # both evaluate the reference's operation order
    assert t_res < t_auto, (n, batch, t_res, t_auto)
