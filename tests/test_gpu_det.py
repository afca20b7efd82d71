"""GPU tests of the determinant beside the inverse (``Inverter.inv_det``, ``det=True`` of ``inv_pointers`` /
``inv_ragged`` / ``inv_diag_blocks``, ``mi32_inv_det_device*``; run with ``-m gpu`` on an MI355X): the register-resident
and the workgroup-resident kernels, uniform and variable-size, fp32 and fp64, with partial pivoting and without.

There is no tolerance anywhere in this file.  The inverse must equal the step-by-step CPU oracle bit for bit
(``np.array_equal``), the status must equal the oracle's, and the determinant -- the (mantissa, exponent) pair of
include/mat_inv_32_c.h -- must equal what the recurrence gives on the pivots of the mirror tests/det_mirror.c, which
tests/test_det_mirror.py holds to the oracle: the mantissas compare as bit patterns, the exponents as integers.
"""
import math

import numpy as np
import pytest

from det_cases import (NOPIVOT_ORDERS, PERMUTATION_ORDERS, WORKGROUP_EDGES, build_mirror, dominant_member, expected,
                       family_members, mixed_wave_orders, permutation_matrix, same_doubles)
from resident_cases import FP64_ORDERS, TIE_ORDERS, big_batch, shared_wave_batch, tie_batch
from vbatch_cases import every_order_members, pack, unpack

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_matrix_inversion_amd as g  # noqa: E402


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return build_mirror(tmp_path_factory.mktemp("det_mirror"))


@pytest.fixture(scope="module")
def inv():
    i = g.Inverter()
    yield i
    i.close()


@pytest.fixture(scope="module")
def inv_nopivot():
    i = g.Inverter(pivoting=False)
    yield i
    i.close()


@pytest.fixture(scope="module")
def every_order(dll):
    """The 511 shuffled members of every order 1 ... 128 and what the mirror expects of them, computed once."""
    mats = every_order_members()
    return mats, expected(dll, mats)


def _oracle_fn(oracle, dtype, pivoting):
    if not pivoting:
        return oracle.matrix_inversion_no_pivots
    return oracle.matrix_inv_32 if dtype == np.float32 else oracle.matrix_inv_64


def _run(inverter, mats, **kw):
    """inv_det on a numpy batch; (inverse or None, status, det_mant, det_exp) as numpy arrays."""
    x, st, mant, exp = inverter.inv_det(torch.from_numpy(np.ascontiguousarray(mats)).cuda(), **kw)
    torch.cuda.synchronize()
    assert mant.dtype == torch.float64 and exp.dtype == torch.int32 and st.dtype == torch.int32
    return (None if x is None else x.cpu().numpy()), st.cpu().numpy(), mant.cpu().numpy(), exp.cpu().numpy()


def _check_batch(oracle, dll, inverter, mats, pivoting=True, tag=None):
    """One uniform call on the batch `mats`; inverse and status against the oracle, the determinant against the mirror."""
    mats = np.ascontiguousarray(mats)
    n = mats.shape[1]
    fn = _oracle_fn(oracle, mats.dtype, pivoting)
    want_x, want_st, want_m, want_e = expected(dll, mats, pivoting)
    x, st, mant, exp = _run(inverter, mats)
    for b, a in enumerate(mats):
        ox, info = fn(a, n, return_info=True)
        assert info["status"] == want_st[b] == st[b], (tag, n, b)
        if st[b] == 0:
            assert np.array_equal(x[b].reshape(-1), ox), (tag, n, b)
            assert np.array_equal(x[b], want_x[b]), (tag, n, b)
    assert same_doubles(mant, want_m), (tag, n, mant, want_m)
    assert np.array_equal(exp, want_e), (tag, n, exp, want_e)
    return st, mant, exp


def test_resident_every_order_fp32(oracle, dll, inv):
    for n in range(1, 65):
        st, mant, _ = _check_batch(oracle, dll, inv, np.stack(family_members(n)), tag="fp32")
        assert not st.any() and (np.abs(mant) >= 0.5).all() and (np.abs(mant) < 1.0).all()


def test_resident_fp64(oracle, dll, inv):
    for n in FP64_ORDERS:
        st, _, _ = _check_batch(oracle, dll, inv, np.stack(family_members(n, np.float64)) * 1.000000001, tag="fp64")
        assert not st.any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_resident_no_pivot(oracle, dll, inv_nopivot, dtype):
    for n in NOPIVOT_ORDERS:
        st, mant, _ = _check_batch(oracle, dll, inv_nopivot, dominant_member(n, dtype)[None], pivoting=False, tag="nopivot")
        assert not st.any() and (mant > 0).all()      # strictly diagonally dominant with a positive diagonal


def test_workgroup_every_order_fp32(oracle, dll, inv):
    for n in range(65, 129):
        st, _, _ = _check_batch(oracle, dll, inv, np.stack(family_members(n)), tag="fp32")
        assert not st.any()


def test_workgroup_fp64_and_no_pivot_at_the_class_edges(oracle, dll, inv, inv_nopivot):
    for n in WORKGROUP_EDGES:
        st, _, _ = _check_batch(oracle, dll, inv, np.stack(family_members(n, np.float64)) * 1.000000001, tag="fp64")
        assert not st.any()
        for dtype in (np.float32, np.float64):
            st, _, _ = _check_batch(oracle, dll, inv_nopivot, dominant_member(n, dtype)[None], pivoting=False,
                                    tag="nopivot")
            assert not st.any()


@pytest.mark.parametrize("n", PERMUTATION_ORDERS)
def test_permutation_matrices(inv, n):
    mats = np.stack([permutation_matrix(n, False), permutation_matrix(n, True)])
    x, st, mant, exp = _run(inv, mats)
    assert not st.any()
    assert np.array_equal(x, mats.transpose(0, 2, 1))           # the inverse of a permutation matrix: its transpose
    assert mant.tolist() == [0.5, -0.5] and exp.tolist() == [1, 1]


@pytest.mark.parametrize("n", [64, 128])
def test_powers_of_two_cannot_overflow(inv, n):
    for k, dtype in ((100, np.float32), (-120, np.float32), (1000, np.float64), (-1000, np.float64)):
        a = np.diag(np.full(n, 2.0 ** k)).astype(dtype)
        x, st, mant, exp = _run(inv, a[None])
        assert not st.any() and np.array_equal(x[0], np.diag(np.full(n, 2.0 ** -k)).astype(dtype)), (n, k)
        assert mant.tolist() == [0.5] and exp.tolist() == [k * n + 1], (n, k, mant, exp)
        sign, logabs = g.slogdet_from_frexp(torch.from_numpy(mant), torch.from_numpy(exp))
        assert sign.item() == 1.0 and logabs.item() == pytest.approx(k * n * math.log(2.0), rel=1e-15)


@pytest.mark.parametrize("n", TIE_ORDERS)
def test_ties(oracle, dll, inv, n):
    _check_batch(oracle, dll, inv, tie_batch(n), tag="ties")


def test_flagged_members_between_good_ones(oracle, dll, inv, inv_nopivot):
    mats, want_st = shared_wave_batch()
    st, mant, exp = _check_batch(oracle, dll, inv, mats, tag="flagged")
    assert st.tolist() == want_st
    assert mant[3] == 0.0 and not np.signbit(mant[3]) and exp[3] == 0          # rank 1: an exactly zero pivot
    assert np.isnan(mant[5]) and exp[5] == 0                                   # a NaN entry
    assert mant[8] == 0.0 and not np.signbit(mant[8]) and exp[8] == 0          # the zero matrix
    good = [b for b in range(9) if want_st[b] == 0]
    assert len(good) == 6 and np.isfinite(mant[good]).all() and (np.abs(mant[good]) >= 0.5).all()
    # pivoting off: a diagonal entry that is, and stays, exactly zero flags the member, and det = 0 does not follow
    for n in (20, 100):
        dom = np.stack([dominant_member(n, np.float32)] * 3)
        dom[1, 1, 1] = dom[1, 1, 0] = 0.0
        st, mant, exp = _check_batch(oracle, dll, inv_nopivot, dom, pivoting=False, tag="nopivot-zero")
        assert st.tolist() == [0, 2, 0] and np.isnan(mant[1]) and exp[1] == 0
        assert mant[0] == mant[2] and exp[0] == exp[2] and np.isfinite(mant[0])


def _run_ragged(inverter, mats, **kw):
    orders, flat = pack(mats)
    plan = inverter.plan_ragged(orders)
    try:
        x, st, (mant, exp) = inverter.inv_ragged(plan, torch.from_numpy(flat).cuda(), det=True, **kw)
        torch.cuda.synchronize()
    finally:
        plan.close()
    return unpack(x.cpu().numpy(), orders), st.cpu().numpy(), mant.cpu().numpy(), exp.cpu().numpy()


def _assert_members(got, st, mant, exp, want, tag):
    want_x, want_st, want_m, want_e = want
    assert np.array_equal(st, want_st), tag
    for b in range(len(want_x)):
        if want_st[b] == 0:
            assert np.array_equal(got[b], want_x[b]), (tag, b, want_x[b].shape)
    bad = [b for b in range(len(want_m)) if not same_doubles(mant[b:b + 1], want_m[b:b + 1]) or exp[b] != want_e[b]]
    assert not bad, (tag, bad[:8], [want_x[b].shape[0] for b in bad[:8]])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_every_order_in_one_call(oracle, dll, inv, every_order, dtype):
    mats, want = every_order
    if dtype == np.float64:
        mats = [m.astype(np.float64) for m in mats]
        want = expected(dll, mats)
    assert sorted({m.shape[0] for m in mats}) == list(range(1, 129)) and not want[1].any()
    fn = _oracle_fn(oracle, dtype, True)
    for m, x in zip(mats[::7], want[0][::7]):                    # the mirror's inverse is the oracle's (a sample here;
        assert np.array_equal(fn(m, m.shape[0]), x.reshape(-1))  # tests/test_det_mirror.py pins it)
    got, st, mant, exp = _run_ragged(inv, mats)
    _assert_members(got, st, mant, exp, want, dtype)             # the determinants land at the caller's indices


def test_groups_of_different_order_share_a_wave(oracle, dll, inv, inv_nopivot):
    orders = mixed_wave_orders()
    assert max(orders) <= 8 and len(set(orders)) == 8
    rng = np.random.default_rng(515)
    mats = [(rng.uniform(-1, 1, (n, n)) + np.sqrt(n) * np.eye(n))[rng.permutation(n)].astype(np.float32) for n in orders]
    got, st, mant, exp = _run_ragged(inv, mats)
    _assert_members(got, st, mant, exp, expected(dll, mats), "mixed wave")
    for b, m in enumerate(mats):
        assert np.array_equal(got[b].reshape(-1), oracle.matrix_inv_32(m, m.shape[0])), b
    dom = [dominant_member(n, np.float64) for n in orders]
    got, st, mant, exp = _run_ragged(inv_nopivot, dom)
    _assert_members(got, st, mant, exp, expected(dll, dom, pivoting=False), "mixed wave, no pivot")


def test_strided_in_place_members_between_nan_padding(dll, inv, every_order):
    mats, want = every_order
    mats, want = mats[::3], tuple(w[::3] for w in want)
    lds = np.array([m.shape[0] + 3 for m in mats], np.int32)
    sizes = np.array([m.shape[0] * ld for m, ld in zip(mats, lds)], np.int64)
    off = np.concatenate(([0], np.cumsum(sizes)[:-1]))
    buf = np.full(int(sizes.sum()), np.nan, np.float32)          # NaN padding: never read, never written
    is_pad = np.ones(buf.size, bool)
    for m, o, ld in zip(mats, off, lds):
        n = m.shape[0]
        buf[o:o + n * ld].reshape(n, ld)[:, :n] = m
        is_pad[o:o + n * ld].reshape(n, ld)[:, :n] = False
    t = torch.from_numpy(buf).cuda()
    ptrs = torch.from_numpy(off * 4 + t.data_ptr()).cuda()
    ld_t = torch.from_numpy(lds).cuda()
    plan = inv.plan_ragged([m.shape[0] for m in mats])
    try:
        st, (mant, exp) = inv.inv_pointers(plan, ptrs, ptrs, torch.float32, lda=ld_t, ldout=ld_t, det=True)
        torch.cuda.synchronize()
    finally:
        plan.close()
    out = t.cpu().numpy()
    got = [out[o:o + m.shape[0] * ld].reshape(m.shape[0], ld)[:, :m.shape[0]] for m, o, ld in zip(mats, off, lds)]
    _assert_members(got, st.cpu().numpy(), mant.cpu().numpy(), exp.cpu().numpy(), want, "strided in place")
    assert np.isnan(out[is_pad]).all()


def test_inv_diag_blocks_with_determinants(oracle, dll, inv):
    orders = [1, 70, 5, 33, 64, 2, 17, 100, 8]
    assert sum(orders) == 300
    rng = np.random.default_rng(52)
    m = np.full((300, 300), np.nan, np.float32)                  # off-block entries are NaN: they are not read
    blocks, off = [], 0
    for n in orders:
        blk = (rng.uniform(-1, 1, (n, n)) + np.sqrt(n) * np.eye(n))[rng.permutation(n)].astype(np.float32)
        m[off:off + n, off:off + n] = blk
        blocks.append(blk)
        off += n
    tm = torch.from_numpy(m).cuda()
    out, st, (mant, exp) = inv.inv_diag_blocks(tm, orders, det=True)
    out0, st0 = inv.inv_diag_blocks(tm, orders)                  # the default form: unchanged shape, same values
    torch.cuda.synchronize()
    assert torch.equal(out, out0) and torch.equal(st, st0)
    x, off, got = out.cpu().numpy(), 0, []
    for n in orders:
        got.append(x[off:off + n, off:off + n])
        off += n
    _assert_members(got, st.cpu().numpy(), mant.cpu().numpy(), exp.cpu().numpy(), expected(dll, blocks), "diag blocks")
    for b, blk in enumerate(blocks):
        assert np.array_equal(got[b].reshape(-1), oracle.matrix_inv_32(blk, blk.shape[0])), b
    # the determinant of the block-diagonal matrix is the product of the blocks': against numpy on the float64 copy
    full = np.where(np.isnan(m), 0.0, m).astype(np.float64)
    sign, logabs = g.slogdet_from_frexp(mant, exp)
    want_sign, want_log = np.linalg.slogdet(full)
    assert sign.prod().item() == want_sign
    assert abs(logabs.sum().item() - want_log) <= 1e-4 * max(1.0, abs(want_log))   # the bound of tests/test_det_mirror.py


def test_determinant_only(dll, inv, every_order):
    for n in (20, 100):
        mats = np.stack(family_members(n))
        x, st, mant, exp = _run(inv, mats)
        none, st1, mant1, exp1 = _run(inv, mats, want_inverse=False)
        assert none is None and np.array_equal(st1, st) and same_doubles(mant1, mant) and np.array_equal(exp1, exp)
        with pytest.raises(ValueError):
            inv.inv_det(torch.from_numpy(mats).cuda(), out=torch.empty(mats.shape, device="cuda"), want_inverse=False)
    # the variable-size call without output pointers; the buffer that would have been the output keeps its sentinel
    mats, want = every_order
    orders, flat = pack(mats)
    a = torch.from_numpy(flat).cuda()
    sentinel = torch.full_like(a, -12345.5)
    plan = inv.plan_ragged(orders)
    try:
        assert plan.packed_pointers(sentinel).numel() == len(mats)            # it would have been the output
        st, (mant, exp) = inv.inv_pointers(plan, plan.packed_pointers(a), None, torch.float32, det=True)
        torch.cuda.synchronize()
        with pytest.raises(ValueError):
            inv.inv_pointers(plan, plan.packed_pointers(a), None, torch.float32)
    finally:
        plan.close()
    assert np.array_equal(st.cpu().numpy(), want[1])
    assert same_doubles(mant.cpu().numpy(), want[2]) and np.array_equal(exp.cpu().numpy(), want[3])
    assert (sentinel == -12345.5).all().item()
    assert torch.equal(a, torch.from_numpy(flat).cuda())                       # the input is unchanged


def test_large_batch(dll, inv):
    n, batch = 8, 70_000                                         # more groups than one grid dimension of 65 535 holds
    mats = big_batch(n, batch)
    _, want_st, want_m, want_e = expected(dll, mats)
    a = torch.from_numpy(mats).cuda()
    x, st, mant, exp = inv.inv_det(a)
    plain, plain_st = inv.inv(a)
    torch.cuda.synchronize()
    assert not want_st.any() and not st.any().item()
    assert torch.equal(x, plain) and torch.equal(st, plain_st)   # the inverse of the plain call bit for bit
    assert same_doubles(mant.cpu().numpy(), want_m)              # every member, none sampled
    assert np.array_equal(exp.cpu().numpy(), want_e)


def test_bad_shapes(inv):
    with pytest.raises(ValueError):
        inv.inv_det(torch.eye(129, device="cuda"))
    with pytest.raises(ValueError):
        inv.inv_det(torch.eye(8, device="cuda", dtype=torch.float16))
    with pytest.raises(ValueError):
        inv.inv_det(torch.eye(8))
    a = torch.eye(8, device="cuda")
    x, st, mant, exp = inv.inv_det(a)                            # (N, N): the inverse is (N, N), the rest has one entry
    torch.cuda.synchronize()
    assert x.shape == (8, 8) and torch.equal(x, a) and st.tolist() == [0] and mant.tolist() == [0.5] and exp.tolist() == [1]
