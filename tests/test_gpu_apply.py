"""GPU tests of Z = blockdiag(X) R for a variable-size batch (``Inverter.apply_ragged`` / ``apply_pointers`` /
``apply_diag_blocks``, ``mi32_apply_device_vbatched*``; run with ``-m gpu`` on an MI355X): mixed orders 1 ... 128 in one
call, fp32 and fp64, groups of different orders inside one wave, column chunks, strided members, in-place calls.

There is no tolerance anywhere in this file.  Z must be a NaN exactly where the restatement tests/apply_mirror.c has one
and equal it bit for bit everywhere else, signs of zeros included (``apply_cases.assert_same_bits``);
tests/test_apply_mirror.py holds the restatement to the exact product.
"""
import functools

import numpy as np
import pytest

from apply_cases import (assert_same_bits, build_apply_mirror, expected_launches, minus_zero_member, mirror_apply,
                         mirror_apply_members, rhs_members, rows_of, underflow_members)
from batch_helpers import median_ms, strided
from resident_cases import dist_matrix
from vbatch_cases import KINDS, bench_members, diag_block_orders, pack, unpack

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_matrix_inversion_amd as g  # noqa: E402

EDGES = [7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128]


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return build_apply_mirror(tmp_path_factory.mktemp("apply_mirror"))


@pytest.fixture(scope="module")
def inv():
    i = g.Inverter()
    yield i
    i.close()


@functools.lru_cache(maxsize=None)
def _every_order_512():
    """Every order 1 ... 128 in the four families, shuffled (read-only: shared by the tests).  Any matrix can be applied:
    the hollow family's zero diagonal is multiplied through."""
    mats = [dist_matrix(KINDS[k], n, 41_000 + 100 * n + k) for n in range(1, 129) for k in range(len(KINDS))]
    assert len(mats) == 512
    return [mats[i] for i in np.random.default_rng(2).permutation(len(mats))]


def _members(orders, seed, dtype=np.float32):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1.0, 1.0, (int(n), int(n))).astype(dtype) for n in orders]


def _ragged(inverter, xs, r, **kw):
    """One apply_ragged call on numpy members and the packed right-hand side r; Z as a numpy array."""
    orders, flat = pack(xs)
    plan = inverter.plan_ragged(orders)
    z = inverter.apply_ragged(plan, torch.from_numpy(flat).cuda(), torch.from_numpy(r).cuda(), **kw)
    torch.cuda.synchronize()
    plan.close()
    assert tuple(z.shape) == r.shape and z.dtype == torch.from_numpy(r).dtype
    return z.cpu().numpy()


def _check(dll, inverter, xs, rs, tag):
    want = mirror_apply_members(dll, xs, rs)
    got = _ragged(inverter, xs, np.concatenate(rs))
    assert_same_bits(got, want, tag)
    return got


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("k", [1, 3])
def test_every_order_in_one_call(dll, inv, k, dtype):
    xs = [x.astype(dtype) for x in _every_order_512()]
    orders = [x.shape[0] for x in xs]
    launches = inv.resolved_apply_ragged(orders, k, np.dtype(dtype).itemsize)
    assert launches == expected_launches(orders, k, np.dtype(dtype).itemsize) and len(launches) == 5
    _check(dll, inv, xs, rhs_members(orders, k, 6000 + k, dtype), f"every order K={k}")


@pytest.mark.parametrize("orders", [EDGES, [1, 7, 2, 6, 3, 5, 4, 8, 1]], ids=["class-edges", "one-wave-class"])
@pytest.mark.parametrize("k", [1, 2])
def test_seams(dll, inv, orders, k):
    """Every lane-class edge in one call; and nine 8-lane groups of different orders: two waves, groups of different
    orders side by side, groups past the end of the range."""
    if orders[0] == 1:
        assert inv.resolved_apply_ragged(orders, k) == [(0, 9, 8, 8)]
    _check(dll, inv, _members(orders, 50 + k), rhs_members(orders, k, 60 + k), "seams")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_minus_zero_beside_a_larger_member(dll, inv, dtype):
    """An order-3 member whose chains end in -0 (the last product is negative and underflows) shares a wave with an
    order-8 member, so its lanes walk five padded terms more: they must leave the sign alone.  The larger member first
    and last, so that the small one sits in either half of the pair."""
    x3, r3 = minus_zero_member(dtype)
    x8, r8 = _members([8], 160, dtype)[0], rhs_members([8], 2, 161, dtype)[0]
    want = mirror_apply(dll, x3, r3)
    assert (want == 0).all() and np.signbit(want[0, 0]) and np.signbit(want[1, 0]) and not np.signbit(want[0, 1])
    for xs, rs, at in (([x3, x8], [r3, r8], 0), ([x8, x3], [r8, r3], 1), ([x8, x3, x8, x3], [r8, r3, r8, r3], 3)):
        got = rows_of(_check(dll, inv, xs, rs, f"-0 at {at}"), [x.shape[0] for x in xs])
        assert_same_bits(got[at], want, f"-0 member at {at}")
    one = _check(dll, inv, [x3, x8], [np.ascontiguousarray(r3[:, :1]), np.ascontiguousarray(r8[:, :1])], "-0, K=1")
    assert np.signbit(one[0, 0]) and np.signbit(one[1, 0])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("orders", [[1, 7, 2, 6, 3, 5, 4, 8, 1], [9, 16, 12, 10, 16], [17, 32, 20, 31, 25], [33, 64, 65, 128]],
                         ids=["8-lanes", "16-lanes", "32-lanes", "wave-and-workgroup"])
def test_subnormals_and_signed_zeros_in_mixed_waves(dll, inv, orders, dtype):
    """Chains that pass through and end in subnormals and zeros of both signs, in groups of different orders side by
    side (the padded terms up to the wave's largest order) and in the classes where a group is a wave or a workgroup."""
    for k in (1, 3):
        xs, rs = underflow_members(orders, k, 170 + k, dtype)
        want = rows_of(mirror_apply_members(dll, xs, rs), orders)
        small = want[int(np.argmin(orders))] if len(set(orders)) > 1 else want[0]
        allz = np.concatenate(want)
        assert ((allz == 0) & np.signbit(allz)).any() and ((allz == 0) & ~np.signbit(allz)).any()
        assert ((np.abs(allz) > 0) & (np.abs(allz) < np.finfo(dtype).tiny)).any()
        assert (small == 0).any()
        _check(dll, inv, xs, rs, f"underflow K={k}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_column_chunks(dll, inv, dtype):
    """K around the chunk width the launch list reports: the result does not depend on the chunking, so it equals the
    single-column calls side by side (and the restatement)."""
    orders = [5, 40, 100]
    kc = inv.resolved_apply_ragged(orders, 1, np.dtype(dtype).itemsize)[0][3]
    assert kc >= 2
    xs = _members(orders, 70, dtype)
    for k in (kc - 1, kc, kc + 1, 3 * kc + 2):
        rs = rhs_members(orders, k, 80 + k, dtype)
        got = _check(dll, inv, xs, rs, f"K={k}")
        single = [_ragged(inv, xs, np.ascontiguousarray(np.concatenate(rs)[:, c])) for c in range(k)]
        assert all(s.shape == (sum(orders),) for s in single)
        assert_same_bits(got, np.stack(single, axis=1), f"K={k} against single columns")


def test_strided_members_and_padding(dll, inv):
    """ldx = n + 3, ldr = K + 2, ldz = K + 1: NaN in all padding of X and R is never read, a sentinel in Z's padding
    survives."""
    k = 3
    orders = [5, 64, 12, 100, 33, 128, 1]
    xs = _members(orders, 90)
    rs = rhs_members(orders, k, 91)
    xbuf, xoff, ldx, _ = strided(xs, 3, np.nan)
    ldr = np.full(len(orders), k + 2, np.int32)
    ldz = np.full(len(orders), k + 1, np.int32)
    roff = np.concatenate(([0], np.cumsum([n * (k + 2) for n in orders])[:-1]))
    zoff = np.concatenate(([0], np.cumsum([n * (k + 1) for n in orders])[:-1]))
    rbuf = np.full(sum(orders) * (k + 2), np.nan, np.float32)
    for r, o, n in zip(rs, roff, orders):
        rbuf[o:o + n * (k + 2)].reshape(n, k + 2)[:, :k] = r
    sentinel = np.float32(-12345.5)
    tx, tr = torch.from_numpy(xbuf).cuda(), torch.from_numpy(rbuf).cuda()
    tz = torch.full((sum(orders) * (k + 1),), float(sentinel), dtype=torch.float32, device="cuda")
    dev = lambda a, dt: torch.from_numpy(np.asarray(a).astype(dt)).cuda()  # noqa: E731
    plan = inv.plan_ragged(orders)
    inv.apply_pointers(plan, dev(xoff * 4 + tx.data_ptr(), np.int64), dev(roff * 4 + tr.data_ptr(), np.int64),
                       dev(zoff * 4 + tz.data_ptr(), np.int64), torch.float32, k, ldx=dev(ldx, np.int32),
                       ldr=dev(ldr, np.int32), ldz=dev(ldz, np.int32))
    torch.cuda.synchronize()
    plan.close()
    zh = tz.cpu().numpy()
    for b, (x, r, o, n) in enumerate(zip(xs, rs, zoff, orders)):
        zb = zh[o:o + n * (k + 1)].reshape(n, k + 1)
        assert_same_bits(zb[:, :k], mirror_apply(dll, x, r), ("strided", b))
        assert (zb[:, k:] == sentinel).all(), b


def test_in_place_and_vector_shape(dll, inv):
    orders = EDGES + [3, 3, 70]
    xs = _members(orders, 100)
    for k in (1, 11):
        rs = rhs_members(orders, k, 101 + k)
        want = mirror_apply_members(dll, xs, rs)
        r = np.concatenate(rs)
        if k == 1:
            r, want = r.reshape(-1), want.reshape(-1)         # a vector keeps its shape
        _, flat = pack(xs)
        plan = inv.plan_ragged(orders)
        tr = torch.from_numpy(r).cuda()
        z = inv.apply_ragged(plan, torch.from_numpy(flat).cuda(), tr, out=tr)
        torch.cuda.synchronize()
        plan.close()
        assert z is tr and tuple(z.shape) == r.shape
        assert_same_bits(z.cpu().numpy(), want, f"in place K={k}")


def test_nan_and_zero_propagation(dll, inv):
    """A NaN in one member's X row and in one member's R column reaches what the restatement says and no other member;
    an exact zero in X is multiplied through (0 * inf is NaN)."""
    k = 2
    orders = [6, 6, 20, 20, 70, 70, 6, 40]
    xs = _members(orders, 110)
    rs = rhs_members(orders, k, 111)
    clean = rows_of(_check(dll, inv, xs, rs, "clean"), orders)
    xs[1][4, 2] = np.nan                     # member 1 shares a wave with members 0 and 6
    rs[3][7, 1] = np.nan                     # member 3 shares a wave with member 2
    xs[4][9, 30] = 0.0
    rs[4][30, 0] = np.inf                    # member 4: row 9 of column 0 is 0 * inf
    got = rows_of(_check(dll, inv, xs, rs, "planted"), orders)
    assert np.isnan(got[1][4]).all() and np.isnan(got[1]).sum() == k
    assert np.isnan(got[3][:, 1]).all() and np.isnan(got[3]).sum() == 20
    assert np.isnan(got[4][9, 0]) and np.isnan(got[4]).sum() == 1 and np.isinf(got[4][:, 0]).sum() == 69
    for b in (0, 2, 5, 6, 7):
        assert_same_bits(got[b], clean[b], ("untouched member", b))


@pytest.mark.parametrize("n,members", [(5, 70_000), (70, 66_000)])
def test_many_members(dll, inv, n, members):
    """More members than a grid's y or z extent holds: 250 distinct X and R, repeated (X and R are only read, so the
    repeats share theirs); every member writes a Z of its own, compared by index."""
    distinct, k = 250, 2
    xs = np.stack(_members([n] * distinct, 120 + n))
    rs = np.stack(rhs_members([n] * distinct, k, 121 + n))
    want = np.stack([mirror_apply(dll, x, r) for x, r in zip(xs, rs)])
    tx, tr = torch.from_numpy(xs).cuda(), torch.from_numpy(rs).cuda()
    tz = torch.zeros((members, n, k), dtype=torch.float32, device="cuda")
    which = torch.arange(members, device="cuda") % distinct
    plan = inv.plan_ragged(np.full(members, n))
    inv.apply_pointers(plan, which * (n * n * 4) + tx.data_ptr(), which * (n * k * 4) + tr.data_ptr(),
                       torch.arange(members, device="cuda") * (n * k * 4) + tz.data_ptr(), torch.float32, k)
    torch.cuda.synchronize()
    plan.close()
    zh = tz.cpu().numpy()
    idx = np.arange(members) % distinct
    nan = np.isnan(want)[idx]
    assert not nan.any() and np.array_equal(zh.view(np.uint32), want.view(np.uint32)[idx])


def test_diag_blocks_dense_and_packed(dll, inv):
    """The 43 diagonal blocks of a 3000 x 3000 matrix: the dense inverse with NaN everywhere off the blocks (only block
    entries are read), and the packed form, which never touches an N x N buffer."""
    orders = diag_block_orders()
    total = sum(orders)
    assert len(orders) == 43 and total == 3000 and max(orders) <= 128
    rng = np.random.default_rng(130)
    m = np.zeros((total, total), np.float32)
    off = np.concatenate(([0], np.cumsum(orders)))
    for b, n in enumerate(orders):
        m[off[b]:off[b] + n, off[b]:off[b] + n] = rng.uniform(-1, 1, (n, n)) + np.sqrt(n) * np.eye(n)
    tm = torch.from_numpy(m).cuda()
    dense, st = inv.inv_diag_blocks(tm, orders)
    packed, st2 = inv.inv_diag_blocks(tm, orders, packed=True)
    torch.cuda.synchronize()
    assert not st.any() and not st2.any()
    assert packed.dim() == 1 and packed.numel() == sum(n * n for n in orders)
    dh = dense.cpu().numpy()
    blocks = [np.ascontiguousarray(dh[off[b]:off[b + 1], off[b]:off[b + 1]]) for b in range(len(orders))]
    for b, blk in enumerate(unpack(packed.cpu().numpy(), orders)):
        assert_same_bits(blk, blocks[b], ("packed inverse", b))
    poisoned = np.full_like(dh, np.nan)
    for b in range(len(orders)):
        poisoned[off[b]:off[b + 1], off[b]:off[b + 1]] = blocks[b]
    tp = torch.from_numpy(poisoned).cuda()
    for k in (1, 3):
        r = rng.uniform(-1, 1, (total,) if k == 1 else (total, k)).astype(np.float32)
        want = mirror_apply_members(dll, blocks, rows_of(r.reshape(total, -1), orders)).reshape(r.shape)
        tr = torch.from_numpy(r).cuda()
        z_dense = inv.apply_diag_blocks(tp, orders, tr)
        z_packed = inv.apply_diag_blocks(packed, orders, tr)
        torch.cuda.synchronize()
        assert tuple(z_dense.shape) == r.shape == tuple(z_packed.shape)
        assert_same_bits(z_dense.cpu().numpy(), want, f"dense K={k}")
        assert_same_bits(z_packed.cpu().numpy(), want, f"packed K={k}")


def test_argument_errors(inv):
    orders = [4, 9, 70]
    plan = inv.plan_ragged(orders)
    x = torch.zeros(plan.flat_size, device="cuda")
    r = torch.zeros(plan.total_rows, 2, device="cuda")
    ptrs = torch.zeros(3, dtype=torch.int64, device="cuda")
    bad = [lambda: inv.apply_ragged(plan, x.double(), r),                                  # dtypes differ
           lambda: inv.apply_ragged(plan, x.half(), r.half()),                             # not float32 / float64
           lambda: inv.apply_ragged(plan, x.cpu(), r),                                     # wrong device
           lambda: inv.apply_ragged(plan, x, r.cpu()),
           lambda: inv.apply_ragged(plan, x[:-1], r),                                      # not the plan's elements
           lambda: inv.apply_ragged(plan, x, r[:-1]),                                      # wrong r shape
           lambda: inv.apply_ragged(plan, x, torch.zeros(plan.total_rows, 2, 2, device="cuda")),
           lambda: inv.apply_ragged(plan, x, torch.zeros(plan.total_rows, 0, device="cuda")),
           lambda: inv.apply_ragged(plan, x, r, out=torch.zeros(plan.total_rows, 3, device="cuda")),
           lambda: inv.apply_ragged(plan, x, x[:plan.total_rows], out=x[:plan.total_rows]),  # out aliases x_flat
           lambda: inv.apply_ragged(plan, x, x, out=x),
           lambda: inv.apply_pointers(plan, ptrs, ptrs, ptrs, torch.float32, 0),            # nrhs < 1
           lambda: inv.apply_pointers(plan, ptrs, ptrs, ptrs, torch.float32, -2),
           lambda: inv.apply_pointers(plan, ptrs, ptrs, ptrs, torch.float16, 1),
           lambda: inv.apply_pointers(plan, ptrs[:2], ptrs, ptrs, torch.float32, 1),
           lambda: inv.apply_pointers(plan, ptrs, ptrs.int(), ptrs, torch.float32, 1),
           lambda: inv.apply_pointers(plan, ptrs, ptrs, ptrs, torch.float32, 1, ldx=ptrs),  # leading dimensions are int32
           lambda: inv.apply_diag_blocks(torch.zeros(5, 5, device="cuda"), [2, 2], torch.zeros(5, device="cuda")),
           lambda: inv.resolved_apply_ragged([4, 129], 1),
           lambda: inv.resolved_apply_ragged([4], 0),
           lambda: inv.resolved_apply_ragged([4], 1, 2)]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {i} was accepted")
    plan.close()
    with pytest.raises(ValueError):
        inv.apply_ragged(plan, x, r)                                                        # a closed plan


def test_stored_inverses_beat_the_elimination(inv):
    """Direction only: applying the stored inverses of 16 384 members of orders 3 ... 64 (K = 1, fp32) takes n^2
    multiply-adds per member where solve_ragged, untouched by this call's existence, repeats an elimination of about
    n^3; losing here is a defect, not noise.  Both times are printed; no ratio is asserted."""
    orders, flat = bench_members(16_384, 3, 64)
    plan = inv.plan_ragged(orders)
    ta = torch.from_numpy(flat).cuda()
    x_flat, st = inv.inv_ragged(plan, ta)
    r = torch.from_numpy(np.random.default_rng(140).uniform(-1, 1, plan.total_rows).astype(np.float32)).cuda()
    z, x, st2 = torch.empty_like(r), torch.empty_like(r), torch.empty(plan.batch, dtype=torch.int32, device="cuda")
    t_apply = median_ms(lambda: inv.apply_ragged(plan, x_flat, r, out=z))
    t_solve = median_ms(lambda: inv.solve_ragged(plan, ta, r, out=x, status=st2))
    assert not st.any() and not st2.any()
    # the two compute the same vector up to rounding: a sanity check of the comparison, not of the bits
    assert float((z - x).abs().max()) < 1e-3
    plan.close()
    print(f"\n apply_ragged {t_apply:.3f} ms   solve_ragged {t_solve:.3f} ms   (16 384 members, orders 3 ... 64, K = 1)")
    assert t_apply < t_solve
