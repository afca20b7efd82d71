"""GPU tests of the variable-size batched inversion (``Inverter.plan_ragged`` / ``inv_ragged`` / ``inv_pointers`` /
``inv_diag_blocks``, ``mi32_inv_device_vbatched``; run with ``-m gpu`` on an MI355X): members of mixed orders 1 ... 128
in one call, packed, strided and in place, fp32 and fp64, with partial pivoting and without.

There is no tolerance anywhere in this file: every member does the arithmetic of the uniform paths, so every member
must equal the step-by-step CPU oracle bit for bit (``np.array_equal``) and every status word must equal the
oracle's.  The oracle's status is asserted first, so no member is ever left out of a comparison.
"""
import ctypes

import numpy as np
import pytest

from batch_helpers import assert_members_equal, median_ms, strided
from vbatch_cases import (BENCH_SHAPES, BIG_MEMBERS, bench_members, big_mixed_members, diag_block_orders,
                          dominant_members, every_order_members, invalid_between_valid, oracle_members, pack, unpack)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_matrix_inversion_amd as g  # noqa: E402


@pytest.fixture(scope="module")
def inv():
    i = g.Inverter(algo="workgroup")
    yield i
    i.close()


@pytest.fixture(scope="module")
def inv_nopivot():
    i = g.Inverter(algo="workgroup", pivoting=False)
    yield i
    i.close()


def _run_packed(inverter, mats):
    """One inv_ragged call on the packed members; (list of inverses, statuses, plan class counts)."""
    orders, flat = pack(mats)
    plan = inverter.plan_ragged(orders)
    try:
        assert plan.batch == len(mats) and np.array_equal(plan.orders, orders) and sum(plan.class_counts) == len(mats)
        x, st = inverter.inv_ragged(plan, torch.from_numpy(flat).cuda())
        torch.cuda.synchronize()
        counts = list(plan.class_counts)
    finally:
        plan.close()
    return unpack(x.cpu().numpy(), orders), st.cpu().numpy().tolist(), counts


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_every_order_in_one_call(oracle, inv, dtype):
    mats = [m.astype(dtype) for m in every_order_members()]
    assert sorted({m.shape[0] for m in mats}) == list(range(1, 129))
    want, want_st = oracle_members(oracle.matrix_inv_32 if dtype == np.float32 else oracle.matrix_inv_64, mats)
    assert want_st == [0] * 511
    got, st, counts = _run_packed(inv, mats)
    assert all(c > 0 for c in counts) and len(counts) == 8, counts
    assert st == [0] * 511, [b for b, s in enumerate(st) if s]
    assert_members_equal(got, want, dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_no_pivot(oracle, inv_nopivot, dtype):
    mats = dominant_members(dtype)
    want, want_st = oracle_members(oracle.matrix_inversion_no_pivots, mats)
    assert want_st == [0] * 128
    got, st, counts = _run_packed(inv_nopivot, mats)
    assert all(c > 0 for c in counts)
    assert st == [0] * 128
    assert_members_equal(got, want, dtype)
    # one member whose (1,1) entry is, and stays, exactly zero: it alone is reported, its neighbours are untouched
    for victim in (next(b for b, m in enumerate(mats) if 3 <= m.shape[0] <= 64),
                   next(b for b, m in enumerate(mats) if m.shape[0] > 64)):
        hit = [m.copy() for m in mats]
        hit[victim][1, 1] = 0.0
        hit[victim][1, 0] = 0.0
        n = hit[victim].shape[0]
        assert oracle.matrix_inversion_no_pivots(hit[victim], n, return_info=True)[1]["status"] == oracle.STATUS_SINGULAR
        got, st, _ = _run_packed(inv_nopivot, hit)
        assert st == [g.MI32_SINGULAR if b == victim else 0 for b in range(128)]
        for b in range(128):
            if b != victim:
                assert np.array_equal(got[b], want[b]), (victim, b)


@pytest.mark.parametrize("n,members", [(20, 301), (100, 77)])
def test_equal_to_the_uniform_paths(inv, n, members):
    rng = np.random.default_rng(4400 + n)
    a = torch.from_numpy((rng.uniform(-1, 1, (members, n, n)) + np.sqrt(n) * np.eye(n)).astype(np.float32)).cuda()
    want, want_st = inv.inv(a)
    plan = inv.plan_ragged([n] * members)
    try:
        x, st = inv.inv_ragged(plan, a.reshape(-1))
        torch.cuda.synchronize()
    finally:
        plan.close()
    assert not want_st.any() and not st.any()
    assert torch.equal(x.view(members, n, n), want)
    a64 = a[:50].double()
    want64, _ = inv.inv(a64)
    plan = inv.plan_ragged([n] * 50)
    try:
        x64, st64 = inv.inv_ragged(plan, a64.reshape(-1))
        torch.cuda.synchronize()
    finally:
        plan.close()
    assert not st64.any() and torch.equal(x64.view(50, n, n), want64)


def test_invalid_members_between_valid_ones(oracle, inv):
    mats, want_st = invalid_between_valid()
    want, oracle_st = oracle_members(oracle.matrix_inv_32, mats)
    assert oracle_st == want_st
    got, st, _ = _run_packed(inv, mats)
    assert st == want_st
    for b in range(len(mats)):
        if want_st[b] == 0:
            assert np.array_equal(got[b], want[b]), b


def test_strided_members_and_untouched_padding(oracle, inv):
    mats = every_order_members()
    want, want_st = oracle_members(oracle.matrix_inv_32, mats)
    assert want_st == [0] * 511
    a_buf, a_off, lda, _ = strided(mats, 3, np.nan)           # NaN in the input padding: never read
    sentinel = np.float32(-12345.5)
    o_buf, o_off, ldo, o_pad = strided([np.zeros_like(m) for m in mats], 5, sentinel)
    o_buf[:] = sentinel
    ta, to = torch.from_numpy(a_buf).cuda(), torch.from_numpy(o_buf).cuda()
    keep = ta.clone()
    plan = inv.plan_ragged([m.shape[0] for m in mats])
    try:
        st = inv.inv_pointers(plan, torch.from_numpy(a_off * 4 + ta.data_ptr()).cuda(),
                              torch.from_numpy(o_off * 4 + to.data_ptr()).cuda(), torch.float32,
                              lda=torch.from_numpy(lda).cuda(), ldout=torch.from_numpy(ldo).cuda())
        torch.cuda.synchronize()
    finally:
        plan.close()
    assert st.cpu().numpy().tolist() == [0] * 511
    out = to.cpu().numpy()
    for b, m in enumerate(mats):
        n = m.shape[0]
        assert np.array_equal(out[o_off[b]:o_off[b] + n * ldo[b]].reshape(n, ldo[b])[:, :n], want[b]), (b, n)
    assert (out[o_pad] == sentinel).all()                       # every output padding element is still the sentinel
    assert torch.equal(ta.view(torch.int32), keep.view(torch.int32))   # the input, NaN padding included, is unchanged


def test_inv_diag_blocks(oracle, inv):
    orders = diag_block_orders(3000)
    assert sum(orders) == 3000 and min(orders) >= 1 and max(orders) <= 128
    rng = np.random.default_rng(5)
    m = np.full((3000, 3000), np.nan, np.float32)               # off-block entries are NaN: they are not read
    blocks, off = [], 0
    for n in orders:
        blk = (rng.uniform(-1, 1, (n, n)) + np.sqrt(n) * np.eye(n))[rng.permutation(n)].astype(np.float32)
        m[off:off + n, off:off + n] = blk
        blocks.append(blk)
        off += n
    want, want_st = oracle_members(oracle.matrix_inv_32, blocks)
    assert want_st == [0] * len(orders)
    out, st = inv.inv_diag_blocks(torch.from_numpy(m).cuda(), orders)
    out2, st2 = inv.inv_diag_blocks(torch.from_numpy(m).cuda(), orders)   # the cached plan
    torch.cuda.synchronize()
    assert not st.any() and not st2.any() and torch.equal(out, out2)
    x = out.cpu().numpy()
    off_block = np.ones((3000, 3000), bool)
    off = 0
    for b, n in enumerate(orders):
        assert np.array_equal(x[off:off + n, off:off + n], want[b]), (b, n)
        off_block[off:off + n, off:off + n] = False
        off += n
    assert (x[off_block] == 0).all()                            # only the block entries are written
    with pytest.raises(ValueError):
        inv.inv_diag_blocks(torch.from_numpy(m).cuda(), orders[:-1])


def test_in_place(inv):
    orders, flat = bench_members(600, 1, 128)
    assert orders.min() <= 64 < orders.max()                    # both kernels
    plan = inv.plan_ragged(orders)
    try:
        a = torch.from_numpy(flat).cuda()
        want, want_st = inv.inv_ragged(plan, a)
        x, st = inv.inv_ragged(plan, a, out=a)
        torch.cuda.synchronize()
    finally:
        plan.close()
    assert x.data_ptr() == a.data_ptr()
    assert not want_st.any() and not st.any() and torch.equal(x, want)


def test_more_members_than_a_grid_dimension_holds(oracle, inv):
    mats = big_mixed_members()
    assert len(mats) == BIG_MEMBERS > 65_535
    want, want_st = oracle_members(oracle.matrix_inv_32, mats)
    assert not any(want_st)
    got, st, _ = _run_packed(inv, mats)
    assert not any(st), [b for b, s in enumerate(st) if s][:8]
    _, want_flat = pack(want)
    _, got_flat = pack(got)
    assert np.array_equal(got_flat, want_flat)                  # every member, none sampled
    assert_members_equal(got, want, "big")


def test_plan_reuse_streams_and_null_status(inv):
    orders, flat0 = bench_members(900, 1, 128, seed=1)
    _, flat1 = bench_members(900, 1, 128, seed=2)
    assert not np.array_equal(flat0, flat1)
    a0, a1 = torch.from_numpy(flat0).cuda(), torch.from_numpy(flat1).cuda()
    fresh = []
    for a in (a0, a1):
        p = inv.plan_ragged(orders)
        fresh.append(inv.inv_ragged(p, a))
        torch.cuda.synchronize()
        p.close()
    plan = inv.plan_ragged(orders)
    x0, st0 = inv.inv_ragged(plan, a0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        x1, st1 = inv.inv_ragged(plan, a1)
    # the plan from another context on the same device
    other = g.Inverter(algo="auto")
    try:
        x2, st2 = other.inv_ragged(plan, a0)
        # d_status = NULL through the raw C entry point: the context keeps the status words itself
        out3 = torch.empty_like(a0)
        other._bind_stream()
        rc = other._lib.mi32_inv_device_vbatched(other._h, plan._p, ctypes.c_void_p(plan.packed_pointers(a0).data_ptr()),
                                                 None, ctypes.c_void_p(plan.packed_pointers(out3).data_ptr()), None, None)
        assert rc == 0
        plan.close()                                            # after the enqueue: safe
        s.synchronize()
        torch.cuda.synchronize()
    finally:
        other.close()
    assert plan._p is None
    for st in (st0, st1, st2, fresh[0][1], fresh[1][1]):
        assert not st.any()
    assert torch.equal(x0, fresh[0][0]) and torch.equal(x1, fresh[1][0])
    assert torch.equal(x2, fresh[0][0]) and torch.equal(out3, fresh[0][0])
    with pytest.raises(ValueError):
        inv.inv_ragged(plan, a0)                                # a closed plan


def test_pointer_cache_by_stream(inv):
    """The member addresses are cached per buffer and per stream: the tensor a stream reads is one that stream wrote."""
    orders = [3, 40, 70, 100]
    plan = inv.plan_ragged(orders)
    try:
        a = torch.zeros(plan.flat_size, device="cuda")
        r = torch.zeros(plan.total_rows, 3, device="cuda")
        for base, get, offsets, step in (
                (a.data_ptr(), lambda: plan.packed_pointers(a), np.cumsum([0] + [n * n for n in orders])[:-1], 4),
                (r.data_ptr(), lambda: plan.row_pointers(r, 3), np.cumsum([0] + orders)[:-1], 3 * 4)):
            first = get()
            assert get() is first
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                other = get()
                assert get() is other
            s.synchronize()
            torch.cuda.synchronize()
            assert other is not first and torch.equal(other, first)
            assert first.dtype == torch.int64 and first.tolist() == [base + int(o) * step for o in offsets]
            assert get() is first
    finally:
        plan.close()


def test_host_side_checks(inv):
    plan = inv.plan_ragged([3, 70, 5])
    try:
        size = 9 + 4900 + 25
        assert plan.flat_size == size and plan.class_counts == [2, 0, 0, 0, 1, 0, 0, 0]
        a = torch.zeros(size, dtype=torch.float32, device="cuda")
        with pytest.raises(ValueError):
            inv.inv_ragged(plan, a[:-1])                                     # the flat length
        with pytest.raises(ValueError):
            inv.inv_ragged(plan, a, out=torch.zeros(size, dtype=torch.float64, device="cuda"))   # a dtype mismatch
        with pytest.raises(ValueError):
            inv.inv_ragged(plan, a.cpu())                                    # a tensor on another device
        with pytest.raises(ValueError):
            inv.inv_ragged(plan, a.to(torch.float16))
        buf = torch.zeros(size + 2, dtype=torch.float32, device="cuda")
        with pytest.raises(ValueError):
            inv.inv_ragged(plan, buf[:size], out=buf[2:])                    # out over a part of the input
        ptrs = torch.zeros(3, dtype=torch.int64, device="cuda")
        with pytest.raises(ValueError):
            inv.inv_pointers(plan, ptrs, ptrs.to(torch.int32), torch.float32)
        with pytest.raises(ValueError):
            inv.inv_pointers(plan, ptrs, ptrs, torch.float32, lda=torch.zeros(3, dtype=torch.int64, device="cuda"))
        with pytest.raises(ValueError):
            inv.inv_pointers(plan, ptrs[:2], ptrs[:2], torch.float32)
        if torch.cuda.device_count() > 1:
            far = g.Inverter(device=1)
            try:
                with pytest.raises(ValueError):
                    far.inv_ragged(plan, a.to("cuda:1"))                     # a plan from another device
            finally:
                far.close()
    finally:
        plan.close()
    for bad in ([], [0], [129], [3, -1], [[3, 4]], [2.5]):
        with pytest.raises(ValueError):
            inv.plan_ragged(bad)


@pytest.mark.parametrize("members,lo,hi", BENCH_SHAPES[:2])
def test_one_call_beats_one_call_per_order(inv, members, lo, hi):
    """Only the direction is asserted (no ratio was known before this feature existed): one ``inv_ragged`` call must
    beat the best a user could do before it -- the same members ALREADY grouped by order into contiguous uniform
    device batches (the host-side gather is left out, which favours the baseline) and one
    ``Inverter(algo="workgroup").inv`` call per distinct order.  Both run in this one process, medians of 5 calls
    after 2 warm-ups.  The ratios measured on an MI355X are in DESIGN.md section 11 and
    profiles/vbatch/mixed_batch.json."""
    orders, flat = bench_members(members, lo, hi)
    mats = unpack(flat, orders)
    distinct = [int(n) for n in np.unique(orders)]
    index = {n: np.nonzero(orders == n)[0] for n in distinct}
    groups = {n: torch.from_numpy(np.stack([mats[b] for b in index[n]])).cuda() for n in distinct}
    outs = {n: torch.empty_like(t) for n, t in groups.items()}
    sts = {n: torch.empty(t.shape[0], dtype=torch.int32, device="cuda") for n, t in groups.items()}

    def per_order():
        for n in distinct:
            inv.inv(groups[n], out=outs[n], status=sts[n])

    a = torch.from_numpy(flat).cuda()
    out = torch.empty_like(a)
    st = torch.empty(members, dtype=torch.int32, device="cuda")
    plan = inv.plan_ragged(orders)
    try:
        t_loop = median_ms(per_order)
        t_one = median_ms(lambda: inv.inv_ragged(plan, a, out=out, status=st))
    finally:
        plan.close()
    print(f"\n{members} members, orders {lo}..{hi}: one call {t_one:.3f} ms, {len(distinct)} calls {t_loop:.3f} ms, "
          f"ratio {t_loop / t_one:.2f}x")
    assert not st.any() and not any(s.any() for s in sts.values())
    got = unpack(out.cpu().numpy(), orders)
    for n in distinct:                                           # equal member by member
        ref = outs[n].cpu().numpy()
        for k, b in enumerate(index[n]):
            assert np.array_equal(got[b], ref[k]), (n, b)
    assert t_one < t_loop, (members, lo, hi, t_one, t_loop)
