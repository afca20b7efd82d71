"""GPU tests of A X = B for a variable-size batch (``Inverter.solve_ragged`` / ``solve_pointers`` / ``solve_diag_blocks``,
``mi32_solve_device_vbatched*``; run with ``-m gpu`` on an MI355X): mixed orders 1 ... 127 in one call on the variable-size
solve kernels, fp32 and fp64, with partial pivoting and without, groups of different orders inside one wave, strided
members, in-place calls, chunked members beside unchunked ones.

There is no tolerance anywhere in this file.  X and the status must equal those of the step-by-step mirror
tests/solve_mirror.c (``np.array_equal``), which tests/test_solve_mirror.py holds to the CPU oracle; X is compared where the
mirror's status is 0.
"""
import functools

import numpy as np
import pytest

from conftest import gate_matrix
from det_cases import family_members
from solve_cases import build_solve_mirror, mirror_solve, rhs
from vbatch_cases import (big_mixed_members, diag_block_orders, dominant_members, every_order_members,
                          invalid_between_valid, pack)
from vsolve_cases import expected_launches, mirror_members, packed_rhs, row_offsets

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_matrix_inversion_amd as g  # noqa: E402


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return build_solve_mirror(tmp_path_factory.mktemp("solve_mirror"))


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


@functools.lru_cache(maxsize=None)
def _every_order_507():
    """every_order_members() without its four order-128 members (read-only: shared by the tests)."""
    mats = [m for m in every_order_members() if m.shape[0] <= 127]
    assert len(mats) == 507
    return mats


def _ragged(inverter, mats, b, **kw):
    """One solve_ragged call on numpy members and the packed right-hand side b; (X, status) as numpy arrays."""
    orders, flat = pack(mats)
    plan = inverter.plan_ragged(orders)
    assert plan.total_rows == int(orders.sum()) == b.shape[0]
    x, st = inverter.solve_ragged(plan, torch.from_numpy(flat).cuda(), torch.from_numpy(b).cuda(), **kw)
    torch.cuda.synchronize()
    plan.close()
    assert st.dtype == torch.int32 and tuple(st.shape) == (len(mats),) and tuple(x.shape) == b.shape
    return x.cpu().numpy(), st.cpu().numpy()


def _check(dll, inverter, mats, b, pivoting=True, tag=None):
    """One call; X and status against the mirror, member by member.  Returns (X, status)."""
    want_x, want_st = mirror_members(dll, mats, b.reshape(b.shape[0], -1), pivoting)
    x, st = _ragged(inverter, mats, b)
    assert np.array_equal(st, want_st), (tag, st, want_st)
    off = row_offsets([m.shape[0] for m in mats])
    x2 = x.reshape(want_x.shape)
    for i in range(len(mats)):
        if want_st[i] == 0:
            assert np.array_equal(x2[off[i]:off[i + 1]], want_x[off[i]:off[i + 1]]), (tag, i, mats[i].shape[0])
    return x, st


@pytest.mark.parametrize("k,launches", [(1, 8), (3, 13)])
def test_every_order_in_one_call(dll, inv, k, launches):
    """Every order 1 ... 127 in every family, shuffled, in one call.  K = 3: orders 126 and 127 are chunked (two and
    three launches of their own), the rest are not."""
    mats = _every_order_507()
    orders = [m.shape[0] for m in mats]
    plan_launches = inv.resolved_solve_ragged(orders, k)
    assert plan_launches == expected_launches(orders, k) and len(plan_launches) == launches
    x, st = _check(dll, inv, mats, packed_rhs(orders, k, 5000 * k), tag=f"K={k}")
    assert not st.any()


@pytest.mark.parametrize("orders,k", [([1, 7, 2, 6, 3, 5, 4, 7, 1], 1),
                                      ([7, 8, 15, 16, 31, 32, 63, 64, 80, 81], 1),
                                      ([7, 8, 15, 16, 31, 32, 63, 64, 80, 81], 2)],
                         ids=["one-wave-class-K1", "class-edges-K1", "class-edges-K2"])
def test_seams_inside_a_wave(dll, inv, orders, k):
    """Nine 8-lane groups of different orders, B in a different lane of each, in two waves with groups past the end;
    and every lane-class edge by width with the register-resident / workgroup-resident edge in one call."""
    mats = [gate_matrix(n, 8100 + 10 * i + k) for i, n in enumerate(orders)]
    if orders[0] == 1:
        assert inv.resolved_solve_ragged(orders, k) == [(0, 9, 0, 1, 8, 0)]
    x, st = _check(dll, inv, mats, packed_rhs(orders, k, 300 + k), tag="seams")
    assert not st.any()


def test_agreement_with_the_uniform_call(inv):
    k, per = 3, 4
    groups = {n: np.stack(family_members(n)) for n in (5, 20, 32, 40, 100)}
    assert all(len(batch) == per for batch in groups.values())
    # interleaved: member i has order (5, 20, 32, 40, 100)[i % 5]
    mats = [groups[n][i] for i in range(per) for n in groups]
    orders = [m.shape[0] for m in mats]
    b = packed_rhs(orders, k, 900)
    x, st = _ragged(inv, mats, b)
    off = row_offsets(orders)
    for n, batch in groups.items():
        idx = [i for i, o in enumerate(orders) if o == n]
        tb = torch.from_numpy(np.stack([b[off[i]:off[i + 1]] for i in idx])).cuda()
        ux, ust = inv.solve(torch.from_numpy(batch).cuda(), tb)
        torch.cuda.synchronize()
        assert np.array_equal(ust.cpu().numpy(), st[idx]) and not st[idx].any(), n
        assert np.array_equal(ux.cpu().numpy(), np.stack([x[off[i]:off[i + 1]] for i in idx])), n


def test_strided_members_between_nan_padding(dll, inv):
    orders, k = [5, 20, 33, 70, 127], 2
    mats = [gate_matrix(n, 8300 + n) for n in orders]
    bs = [rhs(n, k, 8400 + n) for n in orders]
    a_off = np.concatenate(([0], np.cumsum([n * (n + 3) for n in orders])))
    r_off = row_offsets(orders)
    a_buf = np.full(a_off[-1] + 7, np.nan, np.float32)
    b_buf = np.full(r_off[-1] * (k + 2) + 7, np.nan, np.float32)
    for i, n in enumerate(orders):
        a_buf[a_off[i]:a_off[i + 1]].reshape(n, n + 3)[:, :n] = mats[i]
        b_buf[r_off[i] * (k + 2):r_off[i + 1] * (k + 2)].reshape(n, k + 2)[:, :k] = bs[i]
    ta, tb = torch.from_numpy(a_buf).cuda(), torch.from_numpy(b_buf).cuda()
    tx = torch.full((int(r_off[-1]) * (k + 5) + 7,), float("nan"), device="cuda")
    dev = lambda v, dt: torch.tensor(np.asarray(v), dtype=dt, device="cuda")  # noqa: E731
    plan = inv.plan_ragged(orders)
    st = inv.solve_pointers(plan, dev(a_off[:-1] * 4 + ta.data_ptr(), torch.int64),
                            dev(r_off[:-1] * (k + 2) * 4 + tb.data_ptr(), torch.int64),
                            dev(r_off[:-1] * (k + 5) * 4 + tx.data_ptr(), torch.int64), torch.float32, k,
                            lda=dev([n + 3 for n in orders], torch.int32), ldb=dev([k + 2] * 5, torch.int32),
                            ldx=dev([k + 5] * 5, torch.int32))
    torch.cuda.synchronize()
    plan.close()
    assert st.tolist() == [0] * 5
    x_buf = tx.cpu().numpy()
    written = np.zeros(x_buf.size, bool)
    for i, n in enumerate(orders):
        want, want_st = mirror_solve(dll, mats[i], bs[i])
        view = slice(r_off[i] * (k + 5), r_off[i + 1] * (k + 5))
        assert want_st == 0 and np.array_equal(x_buf[view].reshape(n, k + 5)[:, :k], want), n
        written[view].reshape(n, k + 5)[:, :k] = True
    assert np.isnan(x_buf[~written]).all() and not np.isnan(x_buf[written]).any()   # the padding of X is untouched
    assert np.array_equal(ta.cpu().numpy(), a_buf, equal_nan=True)
    assert np.array_equal(tb.cpu().numpy(), b_buf, equal_nan=True)


def test_in_place(dll, inv):
    mats = [gate_matrix(n, 8500 + n) for n in (3, 12, 30, 64, 90, 127, 12)]
    orders, flat = pack(mats)
    for k in (1, 3):           # K = 3: order 127 takes three launches on one in-place buffer
        b = packed_rhs(orders, k, 8600)
        x, st = _check(dll, inv, mats, b, tag="out of place")
        plan = inv.plan_ragged(orders)
        tb = torch.from_numpy(b).cuda()
        x2, st2 = inv.solve_ragged(plan, torch.from_numpy(flat).cuda(), tb, out=tb)
        torch.cuda.synchronize()
        plan.close()
        assert x2.data_ptr() == tb.data_ptr() and np.array_equal(tb.cpu().numpy(), x) and not st2.any().item()
    # a vector keeps its shape
    xv, stv = _ragged(inv, mats, packed_rhs(orders, 1, 8600)[:, 0])
    assert xv.shape == (int(orders.sum()),) and np.array_equal(xv, _ragged(inv, mats, packed_rhs(orders, 1, 8600))[0][:, 0])


def test_flagged_members_between_good_ones(dll, inv):
    mats, want_st = invalid_between_valid()
    orders = [m.shape[0] for m in mats]
    b = packed_rhs(orders, 2, 8700)
    x, st = _check(dll, inv, mats, b, tag="flagged")
    assert st.tolist() == want_st == [2, 0, 2, 0, 0, 0, 0, 0, 2]
    off = row_offsets(orders)
    hit = b.copy()
    hit[off[5] + 13, 1] = np.nan                       # member 5 (order 20) shares its wave with the NaN member 2
    x2, st2 = _check(dll, inv, mats, hit, tag="NaN in B")
    assert st2.tolist() == [2, 0, 2, 0, 0, 2, 0, 0, 2]
    for i in range(9):
        if i != 5:
            assert np.array_equal(x2[off[i]:off[i + 1]], x[off[i]:off[i + 1]], equal_nan=True), i


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_no_pivot(dll, inv_nopivot, dtype):
    mats = [m for m in dominant_members(dtype) if m.shape[0] <= 127]
    orders = [m.shape[0] for m in mats]
    x, st = _check(dll, inv_nopivot, mats, packed_rhs(orders, 2, 8800, dtype), pivoting=False, tag="nopivot")
    assert len(mats) == 127 and not st.any()


def test_fp64_every_order(dll, inv):
    mats = [m.astype(np.float64) * 1.000000001 for m in _every_order_507()]   # entries that are no float32 values
    orders = [m.shape[0] for m in mats]
    x, st = _check(dll, inv, mats, packed_rhs(orders, 1, 8900, np.float64), tag="fp64")
    assert x.dtype == np.float64 and not st.any()


def test_diag_blocks(dll, inv):
    orders = diag_block_orders()
    assert len(orders) == 43 and max(orders) == 127 and sum(orders) == 3000
    off = row_offsets(orders)
    blocks = [gate_matrix(n, 9000 + i) for i, n in enumerate(orders)]
    m = np.full((3000, 3000), np.nan, np.float32)      # only the block entries may be read
    for i, blk in enumerate(blocks):
        m[off[i]:off[i + 1], off[i]:off[i + 1]] = blk
    tm = torch.from_numpy(m).cuda()
    r4 = np.random.default_rng(9100).uniform(-1, 1, (3000, 4)).astype(np.float32)
    plans = []
    for r in (np.ascontiguousarray(r4[:, 0]), r4):
        z, st = inv.solve_diag_blocks(tm, orders, torch.from_numpy(r).cuda())
        torch.cuda.synchronize()
        plans.append(inv._diag_plan[1])
        assert tuple(z.shape) == r.shape and st.tolist() == [0] * 43
        z = z.cpu().numpy().reshape(3000, -1)
        for i, blk in enumerate(blocks):
            want, want_st = mirror_solve(dll, blk, r.reshape(3000, -1)[off[i]:off[i + 1]])
            assert want_st == 0 and np.array_equal(z[off[i]:off[i + 1]], want), (i, orders[i])
    assert plans[0] is plans[1]                         # the same block structure: the cached plan
    out, st = inv.inv_diag_blocks(torch.from_numpy(np.nan_to_num(m)).cuda(), orders)
    assert inv._diag_plan[1] is plans[0]                # ... which inv_diag_blocks shares
    tr = torch.from_numpy(r4).cuda()
    z2, st2 = inv.solve_diag_blocks(tm, orders, tr, out=tr)     # in place
    torch.cuda.synchronize()
    assert z2.data_ptr() == tr.data_ptr() and np.array_equal(tr.cpu().numpy(), z) and not st2.any().item()


def test_many_small_members(dll, inv):
    mats = big_mixed_members()                          # 70 000 members of orders 1 ... 12: 8- and 16-lane groups
    orders = np.array([m.shape[0] for m in mats])
    b = np.random.default_rng(9200).uniform(-1, 1, (int(orders.sum()), 1)).astype(np.float32)
    x, st = _check(dll, inv, mats, b, tag="70 000")    # every member, none sampled
    assert not st.any() and len(mats) > 65_535


def test_many_workgroup_members(dll, inv):
    batch, distinct = 66_000, 64                        # more workgroups than 65 535, orders 65 ... 70
    base = [gate_matrix(65 + s % 6, 9300 + s) * np.float32(0.5 + s / 64) for s in range(distinct)]
    orders = [m.shape[0] for m in base]
    base_b = packed_rhs(orders, 1, 9400)
    want_x, want_st = mirror_members(dll, base, base_b)
    assert not want_st.any() and len({m.tobytes() for m in base}) == distinct
    # tiled on the device: member i is base system i % 64, so the packed batch is the packed base over and over
    a_off = np.concatenate(([0], np.cumsum([n * n for n in orders])))
    r_off = row_offsets(orders)
    whole, rest = divmod(batch, distinct)
    tile = lambda t, cut: torch.cat([t.repeat((whole,) + (1,) * (t.dim() - 1)), t[:cut]])  # noqa: E731
    all_orders = np.concatenate([np.tile(orders, whole), orders[:rest]])
    ta = tile(torch.from_numpy(pack(base)[1]).cuda(), int(a_off[rest]))
    tb = tile(torch.from_numpy(base_b).cuda(), int(r_off[rest]))
    plan = inv.plan_ragged(all_orders)
    assert len(inv.resolved_solve_ragged(all_orders, 1)) == 1
    x, st = inv.solve_ragged(plan, ta, tb)
    torch.cuda.synchronize()
    plan.close()
    assert not st.any().item()
    assert torch.equal(x, tile(torch.from_numpy(want_x).cuda(), int(r_off[rest])))   # each value against its mirror


@pytest.mark.parametrize("k", [1, 3])
def test_cached_addresses_equal_computed_ones(inv, k):
    """``solve_ragged`` takes the member addresses of B and X from the plan's cache: X and the status must equal, bit
    for bit, those of ``solve_pointers`` on addresses computed here -- on the first call, on a second with the same
    buffers (a cache hit), after ten calls with ten other outputs (the cache of eight has been cleared), and in
    place.  Orders on the lane kernels and on the workgroup kernel."""
    orders = [3, 40, 70, 100]
    mats = [gate_matrix(n, 9500 + n) for n in orders]
    ta = torch.from_numpy(pack(mats)[1]).cuda()
    tb = torch.from_numpy(packed_rhs(orders, k, 9600 + k)).cuda()
    a_off = np.concatenate(([0], np.cumsum([n * n for n in orders])[:-1]))
    r_off = row_offsets(orders)[:-1]
    dev = lambda v: torch.tensor(np.asarray(v), dtype=torch.int64, device="cuda")  # noqa: E731
    plan = inv.plan_ragged(orders)
    want = torch.full_like(tb, float("nan"))
    want_st = inv.solve_pointers(plan, dev(a_off * 4 + ta.data_ptr()), dev(r_off * k * 4 + tb.data_ptr()),
                                 dev(r_off * k * 4 + want.data_ptr()), torch.float32, k)
    torch.cuda.synchronize()
    assert want_st.tolist() == [0] * 4 and not torch.isnan(want).any()

    def same(out, b=tb):
        x, st = inv.solve_ragged(plan, ta, b, out=out)
        torch.cuda.synchronize()
        return x is out and torch.equal(x, want) and torch.equal(st, want_st)

    out = torch.full_like(tb, float("nan"))
    assert same(out)
    out.fill_(float("nan"))
    assert same(out)                                             # the same buffers: a cache hit
    others = [torch.full_like(tb, float("nan")) for _ in range(10)]
    assert len({o.data_ptr() for o in others}) == 10
    assert all(same(o) for o in others)                          # more keys than the cache holds
    out.fill_(float("nan"))
    assert same(out)                                             # after the eviction
    in_place = tb.clone()
    assert same(in_place, in_place)                              # out is b
    plan.close()


def test_argument_errors(inv):
    orders = [4, 9, 70]
    mats = [np.eye(n, dtype=np.float32) for n in orders]
    flat = torch.from_numpy(pack(mats)[1]).cuda()
    b = torch.ones(83, 2, device="cuda")
    plan = inv.plan_ragged(orders)
    with_128 = inv.plan_ragged([4, 128])
    with pytest.raises(ValueError):
        inv.solve_ragged(with_128, torch.zeros(16 + 128 * 128, device="cuda"), torch.ones(132, device="cuda"))
    ptrs = torch.zeros(3, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        inv.solve_pointers(plan, ptrs, ptrs, ptrs, torch.float32, 0)         # nrhs = 0
    with pytest.raises(ValueError):
        inv.resolved_solve_ragged(orders, 0)
    with pytest.raises(ValueError):
        inv.resolved_solve_ragged([4, 128], 1)
    with pytest.raises(ValueError):
        inv.solve_ragged(plan, flat, torch.ones(82, 2, device="cuda"))        # wrong length
    with pytest.raises(ValueError):
        inv.solve_ragged(plan, flat, b.double())                              # wrong dtype
    with pytest.raises(ValueError):
        inv.solve_ragged(plan, flat, b.cpu())                                 # wrong device
    with pytest.raises(ValueError):
        inv.solve_ragged(plan, flat, flat[:166].view(83, 2), out=flat)        # out is a_flat
    with pytest.raises(ValueError):
        inv.solve_ragged(plan, flat, b[:, 0].contiguous(), out=flat[2:85])    # out inside a_flat, past its start
    with pytest.raises(ValueError):
        inv.solve_diag_blocks(torch.eye(83, device="cuda"), [4, 9, 69], b)    # orders do not sum to N
    closed = inv.plan_ragged(orders)
    closed.close()
    with pytest.raises(ValueError):
        inv.solve_ragged(closed, flat, b)
    x, st = inv.solve_ragged(plan, flat, b)                                   # and a good call: X = B for A = I
    torch.cuda.synchronize()
    assert torch.equal(x, b) and st.tolist() == [0, 0, 0]
    z, st = inv.solve_diag_blocks(torch.eye(83, device="cuda"), orders, b)
    torch.cuda.synchronize()
    assert torch.equal(z, b) and st.tolist() == [0, 0, 0]
    plan.close()
    with_128.close()
