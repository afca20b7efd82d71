"""GPU tests of the wide workgroup-resident path (``Inverter(algo="wide")``, ``MI32_ALGO=5``; run with ``-m gpu`` on
an MI355X): fp32 orders 129 ... 256, with partial pivoting and without, and the determinant twin.

There is no tolerance anywhere in this file: the path does the sweep's arithmetic element by element, so every
member whose oracle status is 0 must equal the step-by-step CPU oracle bit for bit (``np.array_equal``), and every
status word must equal the oracle's.
"""
import ctypes

import numpy as np
import pytest

import overflow_cases as ovf
import subnormal_cases as sub
from batch_helpers import assert_members_equal, median_ms
from conftest import gate_matrix
from degenerate_cases import zero_column
from det_cases import same_doubles
from det_large_cases import build_mirror_large, expected_pair, mirror_steps
from wide_cases import (BIG_BATCH, BIG_DISTINCT, BIG_ORDER, DET_ORDERS, EDGE_ORDERS, EXTREME_ORDERS, KINDS, MEMBERS, ORDERS,
                        SLOT_ORDERS, TIE_ORDERS, TIMED_SHAPES, big_distinct, big_index, dominant_batch, family_batch,
                        late_singular_batch, mixed_batch, nan_in_last_slab, oracle_batch, overflow_batch, overflow_out,
                        run, slot_batch, subnormal_batch, tie_batch, wide_class, zero_diagonal_entry)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_matrix_inversion_amd as g  # noqa: E402


@pytest.fixture(scope="module")
def inv_wide():
    inv = g.Inverter(algo="wide")
    yield inv
    inv.close()


@pytest.fixture(scope="module")
def inv_wide_nopivot():
    inv = g.Inverter(algo="wide", pivoting=False)
    yield inv
    inv.close()


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return build_mirror_large(tmp_path_factory.mktemp("det_mirror_large"))


# ---- 1. every order ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ORDERS)
def test_every_order_bit_identical_to_oracle(oracle, inv_wide, n):
    assert inv_wide.resolved_algo(n, MEMBERS) == g.ALGO_WIDE == 5
    assert inv_wide.resolved_wide(n) == wide_class(n) + (256,)
    for kind in KINDS:
        mats = family_batch(kind, n)
        want, want_st = oracle_batch(oracle.matrix_inv_32, mats, n)
        got, st = run(inv_wide, mats)
        assert list(want_st) == [0] * MEMBERS and list(st) == [0] * MEMBERS, (kind, n, list(st), list(want_st))
        assert_members_equal(got, want, (kind, n))


# ---- 2. no pivoting ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EDGE_ORDERS)
def test_no_pivot_bit_identical_to_oracle(oracle, inv_wide_nopivot, n):
    assert inv_wide_nopivot.resolved_algo(n, MEMBERS) == g.ALGO_WIDE
    mats = dominant_batch(n)
    want, want_st = oracle_batch(oracle.matrix_inversion_no_pivots, mats, n)
    got, st = run(inv_wide_nopivot, mats)
    assert got.dtype == np.float32
    assert list(want_st) == [0] * MEMBERS and list(st) == [0] * MEMBERS
    assert_members_equal(got, want, n)
    h = zero_diagonal_entry(n, np.float32)
    want_h = oracle.matrix_inversion_no_pivots(h, n, return_info=True)[1]["status"]
    _, st = run(inv_wide_nopivot, h)
    assert int(st[0]) == want_h == oracle.STATUS_SINGULAR


# ---- 3. ties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", TIE_ORDERS)
def test_ties_the_lowest_row_wins(oracle, inv_wide, n):
    mats = tie_batch(n)
    assert mats.shape == (16, n, n)
    want, want_st = oracle_batch(oracle.matrix_inv_32, mats, n)
    assert list(want_st) == [0] * 16   # no member is skipped: a singular draw fails here
    got, st = run(inv_wide, mats)
    assert list(st) == [0] * 16
    assert_members_equal(got, want, n)


# ---- 4. the pivot in every slab and slot ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", SLOT_ORDERS)
def test_the_pivot_in_every_slab_and_slot(oracle, inv_wide, n):
    """Member 1 is the anti-diagonal permutation: the pivot of step r sits in register slot n - 1 - r, so every case of
    the pick / put switch of every slab and every label register is visited.  Member 0 is a signed power-of-two
    permutation.  Both inverses are exact and known in closed form; the oracle agrees with them."""
    mats, exact = slot_batch(n)
    want, want_st = oracle_batch(oracle.matrix_inv_32, mats, n)
    assert list(want_st) == [0, 0] and np.array_equal(want, exact)
    got, st = run(inv_wide, mats)
    assert list(st) == [0, 0]
    assert_members_equal(got, want, n)


# ---- 5. invalid members, late singularity, NaN in the last slab -----------------------------------------------------
def _statuses_and_valid_members(oracle, inv, mats, want_st=None):
    n = mats.shape[1]
    want, oracle_st = oracle_batch(oracle.matrix_inv_32, mats, n)
    if want_st is not None:
        assert list(oracle_st) == want_st
    got, st = run(inv, mats)
    assert list(st) == list(oracle_st), (list(st), list(oracle_st))
    for b in range(len(mats)):
        if oracle_st[b] == 0:
            assert np.array_equal(got[b], want[b]), b
    return list(oracle_st)


def test_invalid_members_among_valid_ones(oracle, inv_wide):
    """Members 2 (rank 1), 4 (a NaN) and 6 (all zero) are invalid; their neighbours must not notice."""
    mats, want_st = mixed_batch(200)
    assert mats.shape == (7, 200, 200)
    _statuses_and_valid_members(oracle, inv_wide, mats, want_st)


@pytest.mark.parametrize("n", EXTREME_ORDERS)
def test_late_singularity(oracle, inv_wide, n):
    """A zero LAST column (the bad pivot is met at step n - 1) and a duplicated row (status 0, a huge inverse)."""
    _statuses_and_valid_members(oracle, inv_wide, late_singular_batch(n), [0, 2, 0, 0, 0])


def test_nan_input_in_the_last_slab(oracle, inv_wide):
    _statuses_and_valid_members(oracle, inv_wide, nan_in_last_slab(), [0, 2, 0])


# ---- 6. gradual underflow and output overflow -----------------------------------------------------------------------
@pytest.mark.parametrize("pivoting", [True, False], ids=["pivot", "nopivot"])
@pytest.mark.parametrize("n", EXTREME_ORDERS)
def test_gradual_underflow(oracle, inv_wide, inv_wide_nopivot, n, pivoting):
    """``down``: the input is subnormal; ``up``: the inverse is.  Held to the plain oracle (this path skips an exact-zero
    multiplier as the sweep does)."""
    inv = inv_wide if pivoting else inv_wide_nopivot
    mats, names = subnormal_batch(n, pivoting)
    want, want_st = oracle_batch(oracle.matrix_inv_32 if pivoting else oracle.matrix_inversion_no_pivots, mats, n)
    got, st = run(inv, mats)
    assert list(want_st) == [0] * len(mats) and list(st) == [0] * len(mats)
    for b, name in enumerate(names):
        what = mats[b] if name.endswith("down") else want[b]   # what is compared is subnormal
        assert sub.share_subnormal(what) >= sub.MIN_SHARE, (name, n, sub.share_subnormal(what))
        assert np.isfinite(want[b]).all()
    assert_members_equal(got, want, (n, pivoting))


@pytest.mark.parametrize("pivoting", [True, False], ids=["pivot", "nopivot"])
@pytest.mark.parametrize("n", EXTREME_ORDERS)
def test_output_overflow(oracle, inv_wide, inv_wide_nopivot, n, pivoting):
    """rows_down and block_diag of overflow_cases: status 0 with infinities and NaN in known places of a mostly finite
    inverse, the same places as the plain oracle's (every NaN as one value); with pivoting also overflow_out's recipe
    of subnormal_cases."""
    inv = inv_wide if pivoting else inv_wide_nopivot
    mats, cs = overflow_batch(n, pivoting)
    want = np.stack([ovf.reference(oracle, c, "skip")[0] for c in cs])
    assert [ovf.reference(oracle, c, "skip")[1] for c in cs] == [0] * len(cs)
    for b, c in enumerate(cs):
        finite, infs, nans = ovf.counts(want[b])
        assert finite >= ovf.MIN_FINITE_SHARE and infs > 0 and nans > 0, (c, finite, infs, nans)
    if pivoting:
        a = overflow_out(n)
        x, info = oracle.matrix_inv_32(a, n, return_info=True)
        assert info["status"] == 0
        mats, want = np.concatenate([mats, a[None]]), np.concatenate([want, x.reshape(1, n, n)])
    got, st = run(inv, mats)
    assert list(st) == [0] * len(mats)
    for b in range(len(mats)):
        assert got[b].dtype == want[b].dtype and np.array_equal(got[b], want[b], equal_nan=True), \
            (n, pivoting, b, ovf.difference(got[b], want[b]))


# ---- 7. more members than a grid dimension holds -------------------------------------------------------------------
def test_more_members_than_a_grid_dimension_holds(oracle, inv_wide):
    """Above 65535 members the sweep and blocked paths cannot be launched (the batch index is a grid y / z
    coordinate).  The batch indexes 256 distinct oracle-checked matrices in a shuffled order; every member is
    compared on the device, none sampled."""
    assert BIG_BATCH > 65_535
    distinct = big_distinct()
    want, want_st = oracle_batch(oracle.matrix_inv_32, distinct, BIG_ORDER)
    assert want_st.shape == (BIG_DISTINCT,) and not want_st.any()
    idx = big_index()
    assert idx.shape == (BIG_BATCH,) and set(idx.tolist()) == set(range(BIG_DISTINCT))
    tidx = torch.from_numpy(idx).cuda()
    ta = torch.from_numpy(distinct).cuda()[tidx].contiguous()
    assert ta.shape == (BIG_BATCH, BIG_ORDER, BIG_ORDER)
    x, st = inv_wide.inv(ta)
    torch.cuda.synchronize()
    assert not st.any().item(), torch.nonzero(st)[:8]
    del ta
    tw = torch.from_numpy(want).cuda()[tidx]
    diff = torch.nonzero((x != tw).flatten(1).any(dim=1)).flatten()
    assert diff.numel() == 0 and torch.equal(x, tw), diff[:8]


# ---- 8. asynchronous, pure and deterministic --------------------------------------------------------------------------
def test_asynchronous_pure_and_deterministic(inv_wide):
    n, batch = 200, 300
    a = torch.from_numpy(np.stack([gate_matrix(n, 8600 + b) for b in range(batch)])).cuda()
    keep = a.clone()
    x0, st0 = inv_wide.inv(a)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    out = torch.empty_like(a)
    with torch.cuda.stream(s):
        x1, st1 = inv_wide.inv(a, out=out)
    s.synchronize()
    torch.cuda.synchronize()
    assert x1.data_ptr() == out.data_ptr()
    assert torch.equal(a, keep)                       # the input is not modified
    assert torch.equal(x0, x1) and not st0.any() and not st1.any()
    # the look-ahead switch changes nothing for this path
    inv_wide.set_lookahead(False)
    try:
        x2, _ = inv_wide.inv(a)
        torch.cuda.synchronize()
    finally:
        inv_wide.set_lookahead(True)
    assert torch.equal(x0, x2)
    # d_status = NULL is allowed by the C ABI: the context keeps the status words itself
    out2 = torch.empty_like(a)
    inv_wide._bind_stream()
    rc = inv_wide._lib.mi32_inv_device(inv_wide._h, ctypes.c_void_p(a.data_ptr()), n, batch,
                                       ctypes.c_void_p(out2.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(out2, x0)


# ---- 9. fallbacks --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,algo,resolved", [(40, "resident", 3), (100, "workgroup", 4)])
def test_small_orders_resolve_to_the_other_one_launch_paths(inv_wide, n, algo, resolved):
    assert inv_wide.resolved_algo(n, 9) == resolved == {"resident": g.ALGO_RESIDENT, "workgroup": g.ALGO_WORKGROUP}[algo]
    assert inv_wide.resolved_wide(n) == (0, 0, 256)
    mats = np.stack([gate_matrix(n, 8300 + b) for b in range(9)])
    other = g.Inverter(algo=algo)
    try:
        want, want_st = run(other, mats)
    finally:
        other.close()
    got, st = run(inv_wide, mats)
    assert not st.any() and not want_st.any() and np.array_equal(got, want)


@pytest.mark.parametrize("n,dtype", [(257, np.float32), (300, np.float32), (200, np.float64)], ids=["257", "300", "fp64-200"])
def test_larger_orders_and_fp64_fall_back_to_what_auto_resolves_to(inv_wide, n, dtype):
    a = gate_matrix(n, 8400 + n).astype(dtype)
    elem = np.dtype(dtype).itemsize
    auto = g.Inverter(algo="auto")
    try:
        if elem == 4:
            assert inv_wide.resolved_algo(n, 1) == auto.resolved_algo(n, 1) != g.ALGO_WIDE
        want, want_st = run(auto, a)
    finally:
        auto.close()
    assert inv_wide.resolved_wide(n, elem) == (0, 0, 256)
    got, st = run(inv_wide, a)
    assert got.dtype == dtype and st[0] == want_st[0] == 0
    assert np.array_equal(got, want)


# ---- 10. host entry points -------------------------------------------------------------------------------------------
def test_host_entry_points_select_it_through_the_environment(oracle, monkeypatch):
    monkeypatch.setenv("MI32_ALGO", "5")
    a = gate_matrix(200, 81)
    assert np.array_equal(g.matrix_inv_32(a.reshape(-1), 200), oracle.matrix_inv_32(a, 200))
    mats = np.stack([gate_matrix(150, 8100 + b) for b in range(64)])
    out, st = g.matrix_inv_32_batched(mats)
    want, want_st = oracle_batch(oracle.matrix_inv_32, mats, 150)
    assert not st.any() and not want_st.any() and np.array_equal(out, want)
    b225 = gate_matrix(225, 83)
    got, times = g.fp32_bench(b225.reshape(-1), 225)
    assert np.array_equal(got, oracle.matrix_inv_32(b225, 225))
    assert times["pivot"] > 0 and times["column"] == 0 and times["makeAug"] == 0, times
    # an invalid matrix is the empty array, as on the other paths
    assert g.matrix_inv_32(np.ones(200 * 200, np.float32), 200).size == 0


# ---- 11. the determinant twin ------------------------------------------------------------------------------------------
def _np(t):
    return None if t is None else t.cpu().numpy()


@pytest.mark.parametrize("pivoting", [True, False], ids=["pivot", "nopivot"])
@pytest.mark.parametrize("n", DET_ORDERS)
def test_determinant_beside_the_inverse(oracle, dll, inv_wide, inv_wide_nopivot, n, pivoting):
    """inv_det_any on a wide Inverter runs the det twin: inverse and status are inv's bit for bit, the pair follows the
    inv_det recurrence over the pivots of the step-by-step mirror, want_inverse=False stores no inverse, and a singular
    member gives (0.0, 0) with pivoting and (NaN, 0) without."""
    inv = inv_wide if pivoting else inv_wide_nopivot
    assert inv.resolved_algo(n, 4) == g.ALGO_WIDE
    if pivoting:
        mats = np.concatenate([family_batch("gate", n, 2), family_batch("hollow", n, 1), zero_column(n, n - 1, 4600 + n)[None]])
    else:
        mats = np.concatenate([dominant_batch(n), zero_diagonal_entry(n, np.float32)[None]])
    t = torch.from_numpy(np.ascontiguousarray(mats)).cuda()
    x0, st0 = inv.inv(t)
    x, st, mant, exp = inv.inv_det_any(t)
    none, st2, mant2, exp2 = inv.inv_det_any(t, want_inverse=False)
    torch.cuda.synchronize()
    assert none is None
    assert mant.dtype == torch.float64 and exp.dtype == torch.int32
    x0, st0, x, st, mant, exp, st2, mant2, exp2 = map(_np, (x0, st0, x, st, mant, exp, st2, mant2, exp2))
    assert np.array_equal(st, st0) and np.array_equal(st2, st0)
    assert x.tobytes() == x0.tobytes(), "inv_det_any's inverse is not inv's"
    want_m, want_e = [], []
    fn = oracle.matrix_inv_32 if pivoting else oracle.matrix_inversion_no_pivots
    for b, a in enumerate(mats):
        mx, mst, piv, swp = mirror_steps(dll, a, pivoting)
        m, e = expected_pair(a, piv, swp, pivoting)
        want_m.append(m)
        want_e.append(e)
        assert st[b] == mst == fn(a, n, return_info=True)[1]["status"], (b, st[b], mst)
        if mst == 0:
            assert np.array_equal(x[b], mx), b
    print(n, pivoting, "mant", mant, "exp", exp)
    assert list(st) == [0] * (len(mats) - 1) + [2]
    assert same_doubles(mant, np.array(want_m)) and np.array_equal(exp, np.array(want_e, np.int32)), (mant, want_m, exp, want_e)
    assert same_doubles(mant2, mant) and np.array_equal(exp2, exp)
    # the singular member
    assert exp[-1] == 0 and (mant[-1] == 0.0 and not np.signbit(mant[-1]) if pivoting else np.isnan(mant[-1]))


def test_inv_det_keeps_its_limit_of_128(inv_wide):
    a = torch.from_numpy(gate_matrix(129, 1)).cuda()
    with pytest.raises(ValueError):
        inv_wide.inv_det(a)
    dm = torch.empty(1, dtype=torch.float64, device="cuda")
    de = torch.empty(1, dtype=torch.int32, device="cuda")
    out = torch.empty_like(a)
    rc = inv_wide._lib.mi32_inv_det_device(inv_wide._h, ctypes.c_void_p(a.data_ptr()), 129, 1, ctypes.c_void_p(out.data_ptr()),
                                           None, ctypes.c_void_p(dm.data_ptr()), ctypes.c_void_p(de.data_ptr()))
    assert rc == g.MI32_BAD_SHAPE


# ---- 12. the direction of the timing ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n,batch", TIMED_SHAPES)
def test_faster_than_the_path_auto_resolves_to(inv_wide, n, batch):
    """Only the direction is asserted (no ratio was known before this path existed): for this batch one wide launch
    must beat what AUTO does today, the blocked path, which this change does not touch and which therefore stands in
    for the parent commit.  Both are timed in this one process, medians of 5 calls after 2 warm-ups, AUTO with its
    workspace reserved first.  (256, 1024) is deliberately not asserted: the wide path loses there; the ratios measured
    on an MI355X are in DESIGN.md section 17 and profiles/wide/wide_batch.json."""
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
    assert inv_wide.resolved_algo(n, batch) == g.ALGO_WIDE
    t_wide = median_ms(lambda: inv_wide.inv(a, out=out, status=st))
    assert not st.any()
    print(f"\nn={n} batch={batch}: wide {t_wide:.3f} ms, auto {t_auto:.3f} ms, ratio {t_auto / t_wide:.2f}x")
    assert torch.equal(out, x_auto)      # both evaluate the reference's operation order
    assert t_wide < t_auto, (n, batch, t_wide, t_auto)
