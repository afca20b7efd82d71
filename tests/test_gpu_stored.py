"""GPU tests of block inverses stored in a per-member format and applied from that store (``Inverter.block_stats`` /
``store_inverses`` / ``apply_stored`` / ``inv_csr_blocks_adaptive``, ``mi32_*_device`` of include/mat_inv_32_stored.h;
run with ``-m gpu`` on an MI355X).

There is no tolerance in this file except in ``test_adaptive_setup_end_to_end``, which says where.  Stored bytes equal
the NumPy restatement (tests/stored_cases.py) byte for byte; statistics equal it bit for bit; Z is a NaN exactly where
the expectation has one and has its bits everywhere else (``apply_cases.assert_same_bits``), the expectation being
tests/apply_mirror.c, or ``apply_ragged`` itself, on the NumPy-widened members."""
import functools

import numpy as np
import pytest

import csr_cases as cc
import stored_cases as sc
from apply_cases import (assert_same_bits, build_apply_mirror, minus_zero_member, mirror_apply, mirror_apply_members,
                         rhs_members, rows_of)
from batch_helpers import strided
from vbatch_cases import pack, unpack

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_matrix_inversion_amd as g  # noqa: E402

DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
EDGES = [7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128]


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return build_apply_mirror(tmp_path_factory.mktemp("apply_mirror"))


@pytest.fixture(scope="module")
def inv():
    i = g.Inverter()
    yield i
    i.close()


def dev(a, dt=None):
    a = np.asarray(a)
    return torch.from_numpy(a if dt is None else a.astype(dt)).cuda()


@functools.lru_cache(maxsize=None)
def _every_order(dtype):
    """(members, formats, widened members): every order 1 ... 128 twice, shuffled, entries inside float16's normal
    range, formats cycling over the order-sorted list so that every lane class holds every format and neighbours in a
    wave differ (read-only: shared by the tests)."""
    orders = np.random.default_rng(11).permutation(np.repeat(np.arange(1, 129), 2))
    xs = sc.members_in_range(orders, 12, dtype)
    formats = sc.cycling_formats(orders, dtype)
    for top, lo in zip((8, 16, 32, 64, 128), (0, 8, 16, 32, 64)):
        inside = formats[(orders > lo) & (orders <= top)]
        assert set(inside.tolist()) == set(sc.codes_of(dtype)), top
    wide = [sc.roundtrip(x, int(f)) for x, f in zip(xs, formats)]
    assert any((w != x).any() for w, x in zip(wide, xs))
    return xs, formats, wide


def _store(inv, xs, formats, **kw):
    """(plan, stored) of the packed members."""
    orders, flat = pack(xs)
    plan = inv.plan_ragged(orders)
    return plan, inv.store_inverses(plan, dev(flat), formats, **kw)


def _apply(inv, xs, formats, rs, **kw):
    plan, stored = _store(inv, xs, formats)
    r = np.concatenate(rs)
    z = inv.apply_stored(stored, dev(r), **kw)
    torch.cuda.synchronize()
    plan.close()
    assert tuple(z.shape) == r.shape and z.dtype == dev(r).dtype
    return z.cpu().numpy()


def _check_apply(dll, inv, xs, formats, rs, tag):
    wide = [sc.roundtrip(x, int(f)) for x, f in zip(xs, formats)]
    got = _apply(inv, xs, formats, rs)
    assert_same_bits(got, mirror_apply_members(dll, wide, rs), tag)
    return got


def _same_stored(got, members, formats, tag, gaps=True):
    """The downloaded store against the restatement: a stored NaN is a NaN (its payload is free), every other byte is
    equal, gaps included (they keep the fill; ``gaps=False``: a buffer the call allocated, whose gaps hold anything)."""
    want = sc.store_bytes(members, formats)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    dtype = members[0].dtype
    free = np.zeros(want.size, bool)
    off, _ = sc.offsets([m.shape[0] for m in members], formats, dtype)
    if not gaps:
        free |= sc.gap_mask([m.shape[0] for m in members], formats, dtype)
    for m, f, o in zip(members, formats, off):
        nan = np.isnan(m).reshape(-1)
        if nan.any():
            nb = sc.elem_bytes(int(f), dtype)
            kind = {sc.NATIVE: dtype, sc.FLOAT32: np.float32, sc.FLOAT16: np.float16, sc.BFLOAT16: np.uint16}[int(f)]
            back = sc.widen(got[o:o + m.size * nb].view(kind), int(f), np.float64)
            assert np.isnan(back[nan]).all(), (tag, "a NaN must stay a NaN")
            free[o:o + m.size * nb] = np.repeat(nan, nb)
    bad = (got != want) & ~free
    assert not bad.any(), (tag, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())


# ---- stored bytes -----------------------------------------------------------------------------------------------------
@DTYPES
def test_stored_bytes_of_every_order(inv, dtype):
    """Strided sources between NaN padding into a store pre-filled with 0xA5: the bytes are the restatement's and every
    gap byte keeps the fill."""
    xs, formats, _ = _every_order(dtype)
    orders = [x.shape[0] for x in xs]
    buf, off, ld, _ = strided(xs, 3, np.nan)
    size = sc.offsets(orders, formats, dtype)[1]
    gap = sc.gap_mask(orders, formats, dtype)
    assert gap.any() and size % 8 == 0
    data = torch.full((size,), sc.FILL, dtype=torch.uint8, device="cuda")
    tb = dev(buf)
    plan = inv.plan_ragged(orders)
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    stored = inv.store_inverses_pointers(plan, dev(off * buf.itemsize + tb.data_ptr(), np.int64), tdt, formats,
                                         dev(ld, np.int32), data=data)
    torch.cuda.synchronize()
    assert stored.data is data and stored.nbytes == size and stored.native_nbytes == sum(n * n for n in orders) * buf.itemsize
    assert stored.counts == tuple(int((formats == c).sum()) for c in range(4)) and stored.nbytes < stored.native_nbytes
    assert np.array_equal(stored.offsets.cpu().numpy(), sc.offsets(orders, formats, dtype)[0])
    got = data.cpu().numpy()
    _same_stored(got, xs, formats, "strided")
    assert (got[gap] == sc.FILL).all()
    # the packed form allocates its own buffer: the member bytes are the same
    packed = inv.store_inverses(plan, dev(pack(xs)[1]), dev(formats, np.int32))
    torch.cuda.synchronize()
    plan.close()
    assert packed.data.numel() == size and np.array_equal(packed.data.cpu().numpy()[~gap], got[~gap])


@DTYPES
def test_special_values_in_every_format(dll, inv, dtype):
    """Ties, range edges, subnormals, +-0, +-inf and a NaN in every format, beside an ordinary member of another format
    in the same wave: the stored bytes, and Z from them."""
    special = sc.special_values(dtype)
    plain = sc.members_in_range([8], 21, dtype)[0]
    codes = sc.codes_of(dtype)
    for code in codes:
        other = codes[(codes.index(code) + 1) % len(codes)]
        for xs, formats in (([special, plain], [code, other]), ([plain, special, plain], [other, code, other])):
            plan, stored = _store(inv, xs, formats, data=torch.full((4096,), sc.FILL, dtype=torch.uint8, device="cuda"))
            torch.cuda.synchronize()
            plan.close()
            size = sc.offsets([8] * len(xs), formats, dtype)[1]
            _same_stored(stored.data.cpu().numpy()[:size], xs, np.array(formats), ("special", code))
            assert (stored.data.cpu().numpy()[size:] == sc.FILL).all()
            for k in (1, 2):
                rs = rhs_members([8] * len(xs), k, 22 + k, dtype)
                got = _check_apply(dll, inv, xs, formats, rs, ("special", code, k))
                assert np.isnan(got).any() and not np.isnan(rows_of(got, [8] * len(xs))[0 if xs[0] is plain else 1]).any()


# ---- apply ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,k", [(np.float32, 1), (np.float32, 3), (np.float32, 9), (np.float64, 1), (np.float64, 3),
                                     (np.float64, 5)])
def test_apply_every_order_in_one_call(dll, inv, dtype, k):
    """A full column chunk followed by a one-column chunk at K = 9 (fp32) and 5 (fp64)."""
    xs, formats, wide = _every_order(dtype)
    orders = [x.shape[0] for x in xs]
    rs = rhs_members(orders, k, 30 + k, dtype)
    assert len(inv.resolved_apply_ragged(orders, k, np.dtype(dtype).itemsize)) == 5
    assert_same_bits(_apply(inv, xs, formats, rs), mirror_apply_members(dll, wide, rs), f"every order K={k}")


@DTYPES
@pytest.mark.parametrize("orders", [[1, 7, 2, 6, 3, 5, 4, 8, 1], EDGES], ids=["one-wave-class", "class-edges"])
def test_seams(dll, inv, orders, dtype):
    """Nine 8-lane groups of different orders with a different format on each neighbour (two waves, groups past the
    end); every lane-class edge."""
    codes = sc.codes_of(dtype)
    xs = sc.members_in_range(orders, 40, dtype)
    for shift in range(len(codes)):
        formats = [codes[(i + shift) % len(codes)] for i in range(len(orders))]
        assert all(a != b for a, b in zip(formats, formats[1:]))
        for k in (1, 2):
            _check_apply(dll, inv, xs, formats, rhs_members(orders, k, 41 + k, dtype), ("seams", shift, k))


@DTYPES
def test_minus_zero_beside_a_member_of_another_format(dll, inv, dtype):
    """The order-3 member whose chains end in -0 beside an order-8 member of another format in one wave: the member
    of apply_cases in the formats that hold its entries, and one of the same pattern whose entries every format holds
    (the underflow then comes from R)."""
    x3, r3 = minus_zero_member(dtype)
    x8, r8 = sc.members_in_range([8], 50, dtype)[0], rhs_members([8], 2, 51, dtype)[0]
    codes = sc.codes_of(dtype)
    want = mirror_apply(dll, x3, r3)
    assert (want == 0).all() and np.signbit(want[0, 0]) and np.signbit(want[1, 0]) and not np.signbit(want[0, 1])
    for f3 in codes:
        if sc.roundtrip(x3, f3).tolist() != x3.tolist():
            continue  # 2^-80 (fp32) is no float16, 2^-540 (fp64) no narrower format at all: the scaled member below
        for f8 in codes:
            if f8 == f3:
                continue
            for xs, fs, rs, at in (([x3, x8], [f3, f8], [r3, r8], 0), ([x8, x3], [f8, f3], [r8, r3], 1)):
                got = rows_of(_check_apply(dll, inv, xs, fs, rs, ("-0", f3, f8, at)), [m.shape[0] for m in xs])
                assert_same_bits(got[at], want, ("-0 member", f3, f8, at))
    # in every format: powers of two that all of them hold, the products underflowing in R instead
    t = dtype(2.0 ** -10)
    tiny = dtype(2.0 ** -140) if dtype == np.float32 else dtype(2.0 ** -1070)
    xp = np.array([[0, 0, -t], [0, -t, -t], [0, -t, 0]], dtype)
    rp = np.array([[1, 1], [tiny, tiny], [tiny, -tiny]], dtype)
    wantp = mirror_apply(dll, xp, rp)
    assert (wantp == 0).all() and np.signbit(wantp[0, 0]) and np.signbit(wantp[1, 0]) and not np.signbit(wantp[0, 1])
    for f3 in codes:
        assert sc.roundtrip(xp, f3).tolist() == xp.tolist()
        f8 = codes[(codes.index(f3) + 1) % len(codes)]
        for xs, fs, rs, at in (([xp, x8], [f3, f8], [rp, r8], 0), ([x8, xp], [f8, f3], [r8, rp], 1)):
            got = rows_of(_check_apply(dll, inv, xs, fs, rs, ("-0 scaled", f3, at)), [m.shape[0] for m in xs])
            assert_same_bits(got[at], wantp, ("-0 scaled member", f3, at))


@DTYPES
def test_equal_to_apply_ragged(inv, dtype):
    """GPU against GPU: the all-native store gives the bits of apply_ragged on the same X, any other store those of
    apply_ragged on the widened X."""
    xs, formats, wide = _every_order(dtype)
    orders, flat = pack(xs)
    plan = inv.plan_ragged(orders)
    for k in (1, 4):
        r = dev(np.concatenate(rhs_members(orders, k, 60 + k, dtype)))
        native = inv.store_inverses(plan, dev(flat), np.zeros(len(xs), np.int32))
        # (a native fp32 member of odd order ends 4 bytes short of the next multiple of 8)
        assert native.native_nbytes == flat.nbytes and native.nbytes == sc.offsets(orders, [0] * len(xs), dtype)[1]
        assert native.nbytes - flat.nbytes == (4 * int((np.asarray(orders) % 2).sum()) if dtype == np.float32 else 0)
        assert native.counts == (len(xs), 0, 0, 0)
        assert_same_bits(inv.apply_stored(native, r).cpu().numpy(), inv.apply_ragged(plan, dev(flat), r).cpu().numpy(),
                         f"native K={k}")
        mixed = inv.store_inverses(plan, dev(flat), formats)
        assert_same_bits(inv.apply_stored(mixed, r).cpu().numpy(),
                         inv.apply_ragged(plan, dev(pack(wide)[1]), r).cpu().numpy(), f"mixed K={k}")
    plan.close()


# ---- memory rules -----------------------------------------------------------------------------------------------------
def test_in_place_strided_and_aliasing(dll, inv):
    orders = EDGES + [3, 3, 70]
    dtype = np.float32
    xs = sc.members_in_range(orders, 70, dtype)
    formats = sc.cycling_formats(orders, dtype, 1)
    wide = [sc.roundtrip(x, int(f)) for x, f in zip(xs, formats)]
    plan, stored = _store(inv, xs, formats)
    for k in (1, 11):
        rs = rhs_members(orders, k, 71 + k)
        want = mirror_apply_members(dll, wide, rs)
        r = np.concatenate(rs)
        if k == 1:
            r, want = r.reshape(-1), want.reshape(-1)         # a vector keeps its shape
        tr = dev(r)
        z = inv.apply_stored(stored, tr, out=tr)
        assert z is tr and tuple(z.shape) == r.shape
        assert_same_bits(z.cpu().numpy(), want, f"in place K={k}")
    # ldr = K + 2, ldz = K + 1: NaN in R's padding is never read, a sentinel in Z's padding survives
    k = 3
    rs = rhs_members(orders, k, 75)
    roff = np.concatenate(([0], np.cumsum([n * (k + 2) for n in orders])[:-1]))
    zoff = np.concatenate(([0], np.cumsum([n * (k + 1) for n in orders])[:-1]))
    rbuf = np.full(sum(orders) * (k + 2), np.nan, np.float32)
    for r, o, n in zip(rs, roff, orders):
        rbuf[o:o + n * (k + 2)].reshape(n, k + 2)[:, :k] = r
    sentinel = np.float32(-12345.5)
    tr = dev(rbuf)
    tz = torch.full((sum(orders) * (k + 1),), float(sentinel), dtype=torch.float32, device="cuda")
    inv.apply_stored_pointers(stored, dev(roff * 4 + tr.data_ptr(), np.int64), dev(zoff * 4 + tz.data_ptr(), np.int64), k,
                              ldr=dev(np.full(len(orders), k + 2), np.int32), ldz=dev(np.full(len(orders), k + 1), np.int32))
    torch.cuda.synchronize()
    zh = tz.cpu().numpy()
    for b, (x, r, o, n) in enumerate(zip(wide, rs, zoff, orders)):
        zb = zh[o:o + n * (k + 1)].reshape(n, k + 1)
        assert_same_bits(zb[:, :k], mirror_apply(dll, x, r), ("strided", b))
        assert (zb[:, k:] == sentinel).all(), b
    # out inside the store is refused
    inside = stored.data[:plan.total_rows * 4].view(torch.float32)
    with pytest.raises(ValueError, match="out must not alias the matrices"):
        inv.apply_stored(stored, torch.zeros(plan.total_rows, device="cuda"), out=inside)
    with pytest.raises(ValueError, match="out must not alias the matrices"):
        inv.apply_stored(stored, inside, out=inside)
    plan.close()
    with pytest.raises(ValueError, match="expected an open RaggedPlan"):
        inv.apply_stored(stored, torch.zeros(plan.total_rows, device="cuda"))


@pytest.mark.parametrize("n,members", [(5, 70_000), (70, 66_000)])
def test_many_members(dll, inv, n, members):
    """More members than a grid's y or z extent holds: 250 distinct stored X of mixed formats and R, repeated through
    the offsets (the store and R are only read); every member writes a Z of its own, compared by index."""
    distinct, k, dtype = 250, 2, np.float32
    xs = sc.members_in_range([n] * distinct, 80 + n, dtype)
    formats = sc.cycling_formats([n] * distinct, dtype)
    wide = [sc.roundtrip(x, int(f)) for x, f in zip(xs, formats)]
    rs = np.stack(rhs_members([n] * distinct, k, 81 + n))
    want = np.stack([mirror_apply(dll, x, r) for x, r in zip(wide, rs)])
    small_plan, small = _store(inv, xs, formats)
    which = torch.arange(members, device="cuda") % distinct
    plan = inv.plan_ragged(np.full(members, n))
    big = g.StoredInverses(plan, small.dtype, small.formats[which].contiguous(), small.offsets[which].contiguous(),
                           small.data, small.nbytes, small.native_nbytes, small.counts)
    tr = dev(rs)
    tz = torch.zeros((members, n, k), dtype=torch.float32, device="cuda")
    inv.apply_stored_pointers(big, which * (n * k * 4) + tr.data_ptr(),
                              torch.arange(members, device="cuda") * (n * k * 4) + tz.data_ptr(), k)
    torch.cuda.synchronize()
    plan.close()
    small_plan.close()
    idx = np.arange(members) % distinct
    assert not np.isnan(want).any() and np.array_equal(tz.cpu().numpy().view(np.uint32), want.view(np.uint32)[idx])


# ---- statistics -------------------------------------------------------------------------------------------------------
def _same_stats(got, want, tag):
    assert got.shape == want.shape and got.dtype == np.float64
    assert_same_bits(got, want, tag)


@DTYPES
def test_statistics_of_every_order(inv, dtype):
    """Packed, and strided between NaN padding (never read: a NaN would show in all three values)."""
    rng = np.random.default_rng(90)
    orders = rng.permutation(np.arange(1, 129))
    xs = [(rng.standard_normal((n, n)) * 10.0 ** rng.uniform(-6, 6, (n, n))).astype(dtype) for n in orders]
    for x in xs[::5]:
        x[rng.uniform(size=x.shape) < 0.3] = 0          # zeros are no minimum
    want = sc.stats_of(xs)
    assert np.isfinite(want[:, :2]).all() and (want[:, 2] > 0).all()
    plan = inv.plan_ragged(orders)
    _same_stats(inv.block_stats(plan, dev(pack(xs)[1])).cpu().numpy(), want, "packed")
    buf, off, ld, _ = strided(xs, 3, np.nan)
    tb = dev(buf)
    got = inv.block_stats_pointers(plan, dev(off * buf.itemsize + tb.data_ptr(), np.int64),
                                   torch.float32 if dtype == np.float32 else torch.float64, dev(ld, np.int32))
    _same_stats(got.cpu().numpy(), want, "strided")
    plan.close()


@DTYPES
def test_statistics_of_zero_nan_and_infinite_members(inv, dtype):
    orders = [6, 6, 6, 6, 70, 70, 70, 128, 40, 6]
    xs = sc.members_in_range(orders, 95, dtype)
    clean = sc.stats_of(xs)
    xs[1][:] = 0                                  # all zero, -0 included
    xs[1][2, 3] = -0.0
    xs[2][4, 1] = np.nan                          # shares a wave with its neighbours
    xs[5][69, 0] = np.nan
    xs[6][33, 65] = -np.inf                       # the second wave of the workgroup
    xs[7][127, 127] = np.inf
    xs[8][0, 0] = dtype(np.finfo(dtype).smallest_subnormal)
    want = sc.stats_of(xs)
    assert want[1].tolist() == [0.0, 0.0, np.inf] and np.isnan(want[2]).all() and np.isnan(want[5]).all()
    assert want[6, 0] == np.inf and want[6, 1] == np.inf and np.isfinite(want[6, 2]) and want[7, 1] == np.inf
    assert want[8, 2] == float(np.finfo(dtype).smallest_subnormal)
    plan = inv.plan_ragged(orders)
    got = inv.block_stats(plan, dev(pack(xs)[1])).cpu().numpy()
    plan.close()
    _same_stats(got, want, "planted")
    for b in (0, 3, 4, 9):
        assert got[b].tolist() == clean[b].tolist(), b


# ---- the adaptive set-up, end to end ----------------------------------------------------------------------------------
FAMILIES = ("float16", "bfloat16", "kappa 1e3", "kappa 1e8", "singular")


def _with_singular_values(n, lo, rng):
    """An n x n matrix whose singular values fall geometrically from 1 to `lo`."""
    u, _ = np.linalg.qr(rng.standard_normal((n, n)))
    v, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (u * np.geomspace(1.0, lo, n)) @ v.T


@functools.lru_cache(maxsize=None)
def _adaptive_case():
    """A CSR matrix of 2 055 rows whose 60 diagonal blocks of orders 3 ... 64 come from five families in turn, with
    three entries per row outside the blocks.  Diagonally dominant blocks (kappa below 4) scaled by 2^-14, whose
    inverses lie in float16's normal range; the same scaled by 2^-30, whose inverses leave float16's range; blocks with
    kappa_2 = 1e3 and 1e8; blocks with an empty row."""
    rng = np.random.default_rng(7100)
    orders = np.concatenate([rng.integers(3, 65, 55), [3, 64, 17, 33, 48]])
    family = np.arange(orders.size) % len(FAMILIES)
    n = int(orders.sum())
    first = cc.consecutive(orders)
    dense = np.zeros((n, n), np.float64)
    r = np.repeat(np.arange(n), 3)
    dense[r, rng.integers(0, n, r.size)] = cc.values_for(r.size, rng)
    for k, f, fam in zip(orders, first, family):
        dom = rng.uniform(-1, 1, (k, k)) + k * np.eye(k)
        blk = {0: dom * 2.0 ** -14, 1: dom * 2.0 ** -30, 4: dom}.get(fam)
        if blk is None:
            blk = _with_singular_values(k, 1e-3 if fam == 2 else 1e-8, rng)
        blk = blk.astype(np.float32).astype(np.float64)          # the same numbers in both working types
        if fam == 4:
            blk[k // 2] = 0
        else:
            assert (blk != 0).all()
        dense[f:f + k, f:f + k] = blk
    rows, cols = np.nonzero(dense)
    crow, col = cc.csr_from_pairs(n, rows, cols, rng)
    val = dense[cc.rows_of_entries(crow), col]
    blocks = [np.ascontiguousarray(dense[f:f + k, f:f + k]) for k, f in zip(orders, first)]
    return orders, family, crow, col, val, blocks


@DTYPES
def test_adaptive_setup_end_to_end(oracle, inv, dtype):
    """csr_diag_blocks, block_stats, inv_ragged, block_stats, choose_storage, store_inverses in one call.

    The one toleranced assertion of this file: for every member with status 0 whose kappa and absmax are finite,
    |z_stored - z_native|_i <= (u_F + 2 gamma_n)(1 + u_F) (|X| |r|)_i with gamma_n = n u_T / (1 - n u_T), the right side
    in float64: one relative perturbation u_F per entry of X (the rule keeps the entries inside the format's normal
    range) plus the rounding of two chains of n fused multiply-adds.  It needs no measurement; when run on an MI355X the
    largest ratio of the two sides was 0.75 ... 0.79 (printed per K)."""
    orders, family, crow, col, val, blocks = _adaptive_case()
    blocks = [b.astype(dtype) for b in blocks]
    fn = oracle.matrix_inv_32 if dtype == np.float32 else oracle.matrix_inv_64
    want_x, want_st = [], []
    for b in blocks:
        x, info = fn(b, b.shape[0], return_info=True)
        ok = np.asarray(x).size == b.size
        want_x.append(np.asarray(x, dtype).reshape(b.shape) if ok else np.zeros_like(b))
        want_st.append(int(info["status"]))
    want_st = np.array(want_st, np.int32)
    assert (want_st[family == 4] != 0).all() and (want_st[family < 3] == 0).all()
    sa, sx = sc.stats_of(blocks), sc.stats_of(want_x)
    with np.errstate(invalid="ignore", over="ignore"):
        expect = sc.choose(dtype, sa[:, 0] * sx[:, 0], sx[:, 1], sx[:, 2], 0.1, want_st)
    counts = {c: int((expect == c).sum()) for c in range(4)}
    print("\n expected members per format", counts, "by family",
          {FAMILIES[f]: sorted(set(expect[family == f].tolist())) for f in range(5)})
    assert all(counts[c] >= 1 for c in sc.codes_of(dtype)), counts
    assert (expect[family == 4] == sc.NATIVE).all() and (expect[family == 0] == sc.FLOAT16).any()
    assert (expect[family == 1] == sc.BFLOAT16).all()
    assert (expect[family == 2] == (sc.FLOAT32 if dtype == np.float64 else sc.NATIVE)).all()
    assert (expect[(family == 3) & (want_st == 0)] == sc.NATIVE).any()

    a = (dev(crow, np.int64), dev(col, np.int64), dev(val, dtype))
    stored, status, formats = inv.inv_csr_blocks_adaptive(a, orders)
    stored2, _, formats2 = inv.inv_csr_blocks_adaptive(a, orders, tol=1e-3)
    x_native, st_native = inv.inv_csr_blocks(a, orders)
    plan = stored.plan
    got_sa = inv.block_stats(plan, inv.csr_diag_blocks(a, orders)).cpu().numpy()
    got_sx = inv.block_stats(plan, x_native).cpu().numpy()
    torch.cuda.synchronize()
    st, fm = status.cpu().numpy(), formats.cpu().numpy()
    assert np.array_equal(st, want_st) and np.array_equal(st_native.cpu().numpy(), want_st)
    assert_same_bits(got_sa, sa, "statistics of A")
    with np.errstate(invalid="ignore", over="ignore"):
        restated = sc.choose(dtype, got_sa[:, 0] * got_sx[:, 0], got_sx[:, 1], got_sx[:, 2], 0.1, st)
        restated2 = sc.choose(dtype, got_sa[:, 0] * got_sx[:, 0], got_sx[:, 1], got_sx[:, 2], 1e-3, st)
    assert fm.dtype == np.int32 and np.array_equal(fm, restated) and np.array_equal(fm, expect)
    assert np.array_equal(formats2.cpu().numpy(), restated2) and not np.array_equal(restated2, restated)
    assert stored.counts == tuple(counts[c] for c in range(4)) and stored.dtype == x_native.dtype
    xs = [np.array(m) for m in unpack(x_native.cpu().numpy(), orders)]
    _same_stored(stored.data.cpu().numpy(), xs, fm, "adaptive store", gaps=False)
    assert stored.nbytes == sc.offsets(orders, fm, dtype)[1] < stored.native_nbytes == x_native.numel() * x_native.element_size()

    u_t = 2.0 ** -24 if dtype == np.float32 else 2.0 ** -53
    for k in (1, 3):
        rs = rhs_members(orders, k, 7200 + k, dtype)
        r = dev(np.concatenate(rs))
        z_stored = rows_of(inv.apply_stored(stored, r).cpu().numpy(), orders)
        z_native = rows_of(inv.apply_ragged(plan, x_native, r).cpu().numpy(), orders)
        worst = 0.0
        for b, (x, rb) in enumerate(zip(xs, rs)):
            if fm[b] == sc.NATIVE:
                assert_same_bits(z_stored[b], z_native[b], ("native member", b))
                continue
            assert st[b] == 0 and np.isfinite(got_sx[b, 1]) and np.isfinite(got_sa[b, 0] * got_sx[b, 0])
            n = x.shape[0]
            u_f = sc.LIMITS[int(fm[b])][0]
            bound = (u_f + 2 * n * u_t / (1 - n * u_t)) * (1 + u_f) * (np.abs(x.astype(np.float64)) @ np.abs(rb.astype(np.float64)))
            diff = np.abs(z_stored[b].astype(np.float64) - z_native[b].astype(np.float64))
            worst = max(worst, float((diff / bound).max()))
            assert (diff <= bound).all(), (b, int(fm[b]), float((diff / bound).max()))
        print(f" K={k}: largest |z_stored - z_native| / bound = {worst:.3f}")
    plan.close()
    stored2.plan.close()
