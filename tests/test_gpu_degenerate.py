"""GPU tests of late singularity and of exactly invertible structured inputs on every inversion path (run with
``-m gpu`` on an MI355X).  The inputs are those of tests/degenerate_cases.py; tests/test_degenerate_cases.py proves
on the CPU that the oracle gives every status and every exact inverse used here.

There is no tolerance anywhere in this file.  A status word is compared with the literal constant and, wherever the
oracle runs, with the oracle's; a singular member's values are unspecified (include/mat_inv_32_c.h) and never looked
at; a valid member is compared byte for byte, -0.0 stored as +0.0 (``canon``: conftest.canonical_bytes, kept in the
member's dtype), with the generator's written-down inverse or with the oracle's result.
"""
import numpy as np
import pytest

from batch_helpers import strided
from conftest import canonical_bytes, gate_matrix
from degenerate_cases import (OVERFLOW_LIST, block_diagonal, canon, duplicate_rows, exact_families, ones_block, overflow,
                              signed_pow2_permutation, zero_column, zero_row)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_matrix_inversion_amd as g  # noqa: E402

OK, SINGULAR = 0, 2
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])


def _handle(**kw):
    inv = g.Inverter(**kw)
    yield inv
    inv.close()


@pytest.fixture(scope="module")
def inv_sweep():
    yield from _handle(algo="sweep")


@pytest.fixture(scope="module")
def inv_blocked():
    yield from _handle(algo="blocked")


@pytest.fixture(scope="module")
def inv_resident():
    yield from _handle(algo="resident")


@pytest.fixture(scope="module")
def inv_wg():
    yield from _handle(algo="workgroup")


@pytest.fixture(scope="module")
def inv_f64_blocked():
    """{requested block width: handle} of the fp64 blocked path (AUTO, from N = 256 on): the default width and 64."""
    invs = {bw: g.Inverter(algo="auto", block_width=bw) for bw in (0, 64)}
    yield invs
    for inv in invs.values():
        inv.close()


def test_constants(oracle):
    assert g.MI32_OK == oracle.STATUS_OK == OK and g.MI32_SINGULAR == oracle.STATUS_SINGULAR == SINGULAR
    x = np.array([-0.0, 1.0], np.float32)
    assert canon(x) == canonical_bytes(x)


def run(inv, a):
    """Invert a numpy matrix or batch (its dtype is kept) on the device; (inverse, status list)."""
    x, st = inv.inv(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    torch.cuda.synchronize()
    return x.cpu().numpy(), st.cpu().numpy().tolist()


def oracle_step(oracle, a):
    """(inverse (n, n), status) of the step-by-step oracle in a's dtype (fp32 above 300 rows: its cache-blocked
    evaluation, bit-identical for every block width -- tests/test_oracle.py)."""
    n = a.shape[0]
    if a.dtype == np.float64:
        x, info = oracle.matrix_inv_64(a, n, return_info=True)
    elif n <= 300:
        x, info = oracle.matrix_inv_32_inplace(a, n, return_info=True)
    else:
        x, info = oracle.matrix_inv_32_blocked_exact(a, n, 128, return_info=True)
    return x.reshape(n, n), int(info["status"])


def late_singular(n, ks, rows, kb, seed, dtype=np.float32):
    """{name: matrix}: zero_column at every k of ks below n, zero_row at `rows`, one ones_block whose tie is at step kb."""
    base = gate_matrix(n, seed)
    out = {f"zero_column[{k}]": zero_column(n, k, seed, dtype, base) for k in sorted({k for k in ks if 0 <= k < n})}
    out.update({f"zero_row[{r}]": zero_row(n, r, seed, dtype, base) for r in rows})
    out[f"ones_block[{kb}]"] = ones_block(n, min(kb, n - 2), seed + 2, dtype)
    return out


# ---- 1. late singularity, every geometry ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [200, 500, 1000, 1900, 2048, 3000, 4000])
def test_late_singularity_every_fp32_panel_geometry(oracle, inv_blocked, n):
    """One order per panel instance (256 / 512 threads, 512 x 2 / x 4 rows, 1024 x 2 / x 3 / x 4 rows): a zero column at
    the first and last step, on both sides of a sub-panel and of an outer-block boundary; a zero row that fails at the
    last step, among the padded rows; a tie followed by an all-zero candidate column across a sub-panel boundary."""
    assert inv_blocked.resolved_algo(n, 1) == g.ALGO_BLOCKED
    w, bw = inv_blocked.resolved_blocking(n, 1)
    assert 0 < w < bw
    cases = late_singular(n, (0, w - 1, w, bw - 1, bw, n - 1), (0, n - 1), w - 1, 1000 + n)
    assert len(cases) >= 7
    for name, a in cases.items():
        _, st = run(inv_blocked, a)
        assert st == [SINGULAR], (n, w, bw, name)
        if n <= 1024:
            assert oracle_step(oracle, a)[1] == SINGULAR, (n, name)


def test_late_singularity_shared_panel_4200(inv_blocked):
    """4224 padded rows: two workgroups share the first panels.  Row 4199 belongs to the second one."""
    n = 4200
    w, bw = inv_blocked.resolved_blocking(n, 1)
    assert (w, bw) == (16, 256)
    cases = late_singular(n, (0, 15, 16), (n - 1,), 15, 1000 + n)
    assert sorted(cases) == sorted(["zero_column[0]", "zero_column[15]", "zero_column[16]", "zero_row[4199]", "ones_block[15]"])
    for name, a in cases.items():
        _, st = run(inv_blocked, a)
        assert st == [SINGULAR], name


@pytest.mark.parametrize("dtype,n", [(np.float32, 5), (np.float32, 64), (np.float32, 257), (np.float32, 600),
                                     (np.float64, 5), (np.float64, 257)])
def test_late_singularity_sweep(oracle, inv_sweep, n, dtype):
    for name, a in late_singular(n, (0, n // 2, n - 1), (0, n - 1), n // 2, 1100 + n, dtype).items():
        _, st = run(inv_sweep, a)
        assert st == [SINGULAR] and oracle_step(oracle, a)[1] == SINGULAR, (n, name)
        if dtype == np.float32:   # the augmented form, the sweep's own data flow
            assert oracle.matrix_inv_32(a, n, return_info=True)[1]["status"] == SINGULAR


@pytest.mark.parametrize("bw_req", [0, 64])
@pytest.mark.parametrize("n", [256, 300, 700])
def test_late_singularity_fp64_blocked(oracle, inv_f64_blocked, n, bw_req):
    inv = inv_f64_blocked[bw_req]
    bw = inv.resolved_blocking_f64(n)
    assert bw > 0 and (bw_req == 0 or bw == 64)
    for name, a in late_singular(n, (0, bw - 1, bw, n - 1), (0, n - 1), bw - 1, 1200 + n, np.float64).items():
        _, st = run(inv, a)
        want = oracle.matrix_inv_64_blocked(a, n, bw, return_info=True)[1]["status"]
        assert st == [SINGULAR] and want == SINGULAR, (n, bw, name)


# ---- 2. late singularity in a batch ---------------------------------------------------------------------------------
def test_late_singular_members_in_a_blocked_batch(oracle, inv_blocked):
    n, B = 300, 6
    assert inv_blocked.resolved_algo(n, B) == g.ALGO_BLOCKED
    mats = np.stack([gate_matrix(n, 1300 + b) for b in range(B)])
    mats[2] = zero_column(n, 299, 1302)
    mats[4] = zero_row(n, 150, 1304)
    want = [oracle_step(oracle, m) for m in mats]
    assert [s for _, s in want] == [0, 0, 2, 0, 2, 0]
    got, st = run(inv_blocked, mats)
    assert st == [0, 0, 2, 0, 2, 0]
    for b in (0, 1, 3, 5):
        assert canon(got[b]) == canon(want[b][0]), b


def _shared_wave_batch(n, dtype, seed):
    """16 members of order n.  Members 1, 5, 6 have a zero column (k = 0, n // 2, n - 1), member 10 a zero row, member
    13 the ones block: with 8, 4 or 2 matrices per wave each of them shares its wave with valid members."""
    mats = np.stack([gate_matrix(n, seed + b) for b in range(16)]).astype(dtype)
    mats[1] = zero_column(n, 0, seed + 1, dtype)
    mats[5] = zero_column(n, n // 2, seed + 5, dtype)
    mats[6] = zero_column(n, n - 1, seed + 6, dtype)
    mats[10] = zero_row(n, n // 2, seed + 10, dtype)
    mats[13] = ones_block(n, (n - 2) // 2, seed + 13, dtype)
    return mats, [SINGULAR if b in (1, 5, 6, 10, 13) else OK for b in range(16)]


def _check_batch(oracle, inv, mats, want_st, tag):
    want = [oracle_step(oracle, m) for m in mats]
    assert [s for _, s in want] == want_st, tag
    got, st = run(inv, mats)
    assert got.dtype == mats.dtype
    assert st == want_st, (tag, st)
    for b, s in enumerate(want_st):
        if s == OK:
            assert canon(got[b]) == canon(want[b][0]), (tag, b)


@DTYPES
@pytest.mark.parametrize("n", [3, 8, 9, 16, 17, 33, 64])
def test_late_singular_members_in_a_resident_batch(oracle, inv_resident, n, dtype):
    assert inv_resident.resolved_algo(n, 16) == g.ALGO_RESIDENT
    mats, want_st = _shared_wave_batch(n, dtype, 1400 + 20 * n)
    _check_batch(oracle, inv_resident, mats, want_st, (n, dtype))


@DTYPES
@pytest.mark.parametrize("n", [65, 80, 81, 128])
def test_late_singular_members_in_a_workgroup_batch(oracle, inv_wg, n, dtype):
    assert inv_wg.resolved_algo(n, 16) == g.ALGO_WORKGROUP
    mats, want_st = _shared_wave_batch(n, dtype, 1500 + 20 * n)
    _check_batch(oracle, inv_wg, mats, want_st, (n, dtype))


# ---- 3. variable-size batch -----------------------------------------------------------------------------------------
def _run_strided(inv, mats, sentinel):
    """One inv_pointers call over strided members, the output a sentinel-filled buffer; (members, statuses).  Asserts
    that every output padding element is still the sentinel and that the input is unchanged."""
    tdt = torch.float32 if mats[0].dtype == np.float32 else torch.float64
    es = mats[0].dtype.itemsize
    a_buf, a_off, lda, _ = strided(mats, 3, np.nan)            # NaN in the input padding: never read
    o_buf, o_off, ldo, o_pad = strided([np.zeros_like(m) for m in mats], 5, sentinel)
    o_buf[:] = sentinel
    ta, to = torch.from_numpy(a_buf).cuda(), torch.from_numpy(o_buf).cuda()
    keep = ta.clone()
    plan = inv.plan_ragged([m.shape[0] for m in mats])
    try:
        st = inv.inv_pointers(plan, torch.from_numpy(a_off * es + ta.data_ptr()).cuda(),
                              torch.from_numpy(o_off * es + to.data_ptr()).cuda(), tdt,
                              lda=torch.from_numpy(lda).cuda(), ldout=torch.from_numpy(ldo).cuda())
        torch.cuda.synchronize()
    finally:
        plan.close()
    out = to.cpu().numpy()
    assert (out[o_pad] == sentinel).all()
    assert torch.equal(ta.view(torch.int32), keep.view(torch.int32))
    got = [out[o_off[b]:o_off[b] + m.shape[0] * ldo[b]].reshape(m.shape[0], ldo[b])[:, :m.shape[0]]
           for b, m in enumerate(mats)]
    return got, st.cpu().numpy().tolist()


@DTYPES
def test_ragged_call_with_late_singular_members(oracle, inv_wg, dtype):
    """Every order 1 ... 128 once, shuffled; every eighth member has a zero column at a random step or a zero row."""
    rng = np.random.default_rng(1600)
    orders = rng.permutation(np.arange(1, 129))
    mats, want_st = [], []
    for b, n in enumerate(int(n) for n in orders):
        if b % 8 == 3:
            k = int(rng.integers(0, n))
            mats.append(zero_column(n, k, 1600 + b, dtype) if b % 16 == 3 else zero_row(n, k, 1600 + b, dtype))
            want_st.append(SINGULAR)
        else:
            mats.append(gate_matrix(n, 1600 + b).astype(dtype))
            want_st.append(OK)
    assert want_st.count(SINGULAR) == 16
    want = [oracle_step(oracle, m) for m in mats]
    assert [s for _, s in want] == want_st
    got, st = _run_strided(inv_wg, mats, dtype(-12345.5))
    assert st == want_st, [b for b in range(128) if st[b] != want_st[b]]
    for b in range(128):
        if want_st[b] == OK:
            assert canon(got[b]) == canon(want[b][0]), (b, int(orders[b]))


DIAG_ORDERS = [5, 64, 100, 17, 128, 30, 9, 70, 65, 1, 2, 110]


@pytest.mark.parametrize("victim", [2, 3], ids=["workgroup-class", "resident-class"])
def test_inv_diag_blocks_with_one_singular_block(oracle, inv_wg, victim):
    _, blocks = block_diagonal(DIAG_ORDERS, 1700)
    nv = DIAG_ORDERS[victim]
    blocks[victim] = zero_column(nv, nv - 1, 1700 + victim)
    n = sum(DIAG_ORDERS)
    m = np.full((n, n), np.nan, np.float32)                      # off-block entries are NaN: they are not read
    off_block = np.ones((n, n), bool)
    offs = np.concatenate(([0], np.cumsum(DIAG_ORDERS)))
    for b, blk in enumerate(blocks):
        m[offs[b]:offs[b + 1], offs[b]:offs[b + 1]] = blk
        off_block[offs[b]:offs[b + 1], offs[b]:offs[b + 1]] = False
    want = [oracle_step(oracle, blk) for blk in blocks]
    want_st = [SINGULAR if b == victim else OK for b in range(len(blocks))]
    assert [s for _, s in want] == want_st
    out, st = inv_wg.inv_diag_blocks(torch.from_numpy(m).cuda(), DIAG_ORDERS)
    torch.cuda.synchronize()
    assert st.cpu().numpy().tolist() == want_st
    x = out.cpu().numpy()
    assert (x[off_block] == 0).all()                             # a NaN-flooded block does not leak
    for b in range(len(blocks)):
        if b != victim:
            assert canon(x[offs[b]:offs[b + 1], offs[b]:offs[b + 1]]) == canon(want[b][0]), b


def test_block_diagonal_matrix_as_a_whole_and_by_blocks(oracle, inv_wg, inv_blocked):
    """What block-Jacobi relies on: inverting the diagonal blocks one by one is inverting the block-diagonal matrix."""
    a, blocks = block_diagonal(DIAG_ORDERS, 1800)
    n = a.shape[0]
    assert inv_blocked.resolved_algo(n, 1) == g.ALGO_BLOCKED
    ta = torch.from_numpy(a).cuda()
    by_blocks, st = inv_wg.inv_diag_blocks(ta, DIAG_ORDERS)
    whole, st_whole = inv_blocked.inv(ta)
    torch.cuda.synchronize()
    assert not st.any() and st_whole.cpu().numpy().tolist() == [OK]
    xb, xw = by_blocks.cpu().numpy(), whole.cpu().numpy()
    off_block = np.ones((n, n), bool)
    offs = np.concatenate(([0], np.cumsum(DIAG_ORDERS)))
    for b, blk in enumerate(blocks):
        s = slice(offs[b], offs[b + 1])
        want, want_st = oracle_step(oracle, blk)
        assert want_st == OK
        assert canon(xb[s, s]) == canon(xw[s, s]) == canon(want), (b, blk.shape)
        off_block[s, s] = False
    assert (xb[off_block] == 0).all() and (xw[off_block] == 0).all()


# ---- 4. the next call on the same handle is clean -------------------------------------------------------------------
def _then_clean(oracle, inv, singular, valid, tag, want_fn=oracle_step):
    """Invert every singular input (NaN / inf flood the handle's workspace), then every valid one."""
    for a in singular:
        _, st = run(inv, a)
        assert set(st) == {SINGULAR}, tag
    for a in valid:
        got, st = run(inv, a)
        assert set(st) == {OK}, (tag, a.shape)
        for b, m in enumerate(a if a.ndim == 3 else a[None]):
            want, want_st = want_fn(oracle, m)
            assert want_st == OK and canon((got if a.ndim == 3 else got[None])[b]) == canon(want), (tag, a.shape, b)


def _flood(n, seed, dtype=np.float32):
    # a zero pivot at step 0 (1/0 from the first step on: the widest flood) and one at the last step
    return [zero_column(n, 0, seed, dtype), zero_row(n, n - 1, seed + 1, dtype)]


def test_next_call_is_clean_sweep(oracle, inv_sweep):
    _then_clean(oracle, inv_sweep, _flood(257, 1900), [gate_matrix(257, 1902), gate_matrix(100, 1903)], "sweep")
    _then_clean(oracle, inv_sweep, _flood(257, 1904, np.float64),
                [gate_matrix(257, 1905).astype(np.float64), gate_matrix(100, 1906).astype(np.float64)], "sweep64")


def test_next_call_is_clean_blocked(oracle, inv_blocked):
    _then_clean(oracle, inv_blocked, _flood(600, 1910), [gate_matrix(600, 1912), gate_matrix(300, 1913)], "blocked")


def test_next_call_is_clean_fp64_blocked(oracle, inv_f64_blocked):
    inv = inv_f64_blocked[0]

    def mirror(oracle, m):
        n = m.shape[0]
        x, info = oracle.matrix_inv_64_blocked(m, n, inv.resolved_blocking_f64(n), return_info=True)
        return x.reshape(n, n), int(info["status"])
    assert inv.resolved_blocking_f64(300) > 0
    _then_clean(oracle, inv, _flood(700, 1920, np.float64),
                [gate_matrix(700, 1922).astype(np.float64), gate_matrix(300, 1923).astype(np.float64)], "blocked64", mirror)


@DTYPES
def test_next_call_is_clean_resident_and_workgroup(oracle, inv_resident, inv_wg, dtype):
    for inv, n, small in ((inv_resident, 33, 17), (inv_wg, 100, 80)):
        flood = [np.stack([_flood(n, 1930 + 4 * b, dtype)[b % 2] for b in range(16)])]
        valid = [np.stack([gate_matrix(k, 1950 + b) for b in range(16)]).astype(dtype) for k in (n, small)]
        _then_clean(oracle, inv, flood, valid, (n, dtype))


@DTYPES
def test_next_call_is_clean_ragged_plan(oracle, inv_wg, dtype):
    orders = [int(n) for n in np.random.default_rng(1960).integers(1, 129, 40)]
    plan = inv_wg.plan_ragged(orders)
    small = inv_wg.plan_ragged([max(1, n // 2) for n in orders])
    try:
        bad = [zero_column(n, 0, 1960 + b, dtype) if b % 2 else zero_row(n, n - 1, 1960 + b, dtype)
               for b, n in enumerate(orders)]
        _, st = inv_wg.inv_ragged(plan, torch.from_numpy(np.concatenate([m.reshape(-1) for m in bad])).cuda())
        assert st.cpu().numpy().tolist() == [SINGULAR] * 40
        for p in (plan, small):
            mats = [gate_matrix(int(n), 1970 + b).astype(dtype) for b, n in enumerate(p.orders)]
            x, st = inv_wg.inv_ragged(p, torch.from_numpy(np.concatenate([m.reshape(-1) for m in mats])).cuda())
            torch.cuda.synchronize()
            assert st.cpu().numpy().tolist() == [OK] * 40
            flat, off = x.cpu().numpy(), 0
            for b, m in enumerate(mats):
                want, want_st = oracle_step(oracle, m)
                assert want_st == OK and canon(flat[off:off + m.size]) == canon(want), (b, m.shape)
                off += m.size
    finally:
        plan.close()
        small.close()


def test_next_call_is_clean_shared_panel_4200(oracle, inv_blocked):
    """The exchange buffers of the two-workgroup panels hold the singular call's records when the valid call starts."""
    n = 4200
    _, st = run(inv_blocked, zero_column(n, 0, 1980))
    assert st == [SINGULAR]
    a = gate_matrix(n, 40_000)
    got, st = run(inv_blocked, a)
    want, want_st = oracle_step(oracle, a)
    assert st == [OK] and want_st == OK
    assert canonical_bytes(got) == canonical_bytes(want)


# ---- 5. exact families on every path --------------------------------------------------------------------------------
def _check_exact(inv, n, dtype, seed, tag, names=None):
    fam = exact_families(n, seed, dtype, names)
    for name in fam:
        a, x = fam[name]
        got, st = run(inv, a)
        assert got.dtype == dtype and st == [OK], (tag, n, name, st)
        assert canon(got) == canon(x), (tag, n, name, int((got != x).sum()))


@DTYPES
@pytest.mark.parametrize("n", [1, 2, 3, 64, 257])
def test_exact_families_sweep(inv_sweep, n, dtype):
    _check_exact(inv_sweep, n, dtype, 2000, "sweep")


@pytest.mark.parametrize("n", [129, 300, 1000, 2048, 3000, 4200])
def test_exact_families_blocked(inv_blocked, n):
    assert inv_blocked.resolved_algo(n, 1) == g.ALGO_BLOCKED
    # above 2048 rows one input per family: the -0.0 permutation, the diagonal, one bidiagonal
    _check_exact(inv_blocked, n, np.float32, 2100, "blocked", ("perm-0", "diag", "lower") if n > 2048 else None)


@pytest.mark.parametrize("bw_req", [0, 64])
@pytest.mark.parametrize("n", [256, 700])
def test_exact_families_fp64_blocked(inv_f64_blocked, n, bw_req):
    inv = inv_f64_blocked[bw_req]
    assert inv.resolved_blocking_f64(n) > 0
    _check_exact(inv, n, np.float64, 2200, ("blocked64", bw_req))


@pytest.mark.parametrize("n", [64, 512, 640])
def test_exact_families_fp64_no_pivot(n):
    """The no-pivot variant takes the diagonal entry as every pivot: the diagonal and the two bidiagonal families."""
    inv = g.Inverter(algo="blocked", pivoting=False)
    try:
        assert inv.resolved_blocking_f64(n) > 0
        _check_exact(inv, n, np.float64, 2300, "nopivot64", ("diag", "lower", "upper"))
    finally:
        inv.close()


def _exact_batch(n, dtype, seed):
    fam = exact_families(n, seed, dtype)
    return np.stack([a for a, _ in fam.values()]), np.stack([x for _, x in fam.values()]), list(fam)


@DTYPES
@pytest.mark.parametrize("lanes", [8, 16, 32, 64])
def test_exact_families_resident_every_order(inv_resident, lanes, dtype):
    """Every order of one lane class, the five families of an order as one batch."""
    orders = [n for n in range(1, 65) if inv_resident.resolved_resident(n, np.dtype(dtype).itemsize)[0] == lanes]
    assert orders, lanes
    for n in orders:
        assert inv_resident.resolved_algo(n, 5) == g.ALGO_RESIDENT
        a, x, names = _exact_batch(n, dtype, 2400)
        got, st = run(inv_resident, a)
        assert st == [OK] * len(names), (n, st)
        for b, name in enumerate(names):
            assert canon(got[b]) == canon(x[b]), (n, name)


def test_resident_lane_classes_cover_every_order(inv_resident):
    for es in (4, 8):
        assert sorted({inv_resident.resolved_resident(n, es)[0] for n in range(1, 65)}) == [8, 16, 32, 64]


@DTYPES
@pytest.mark.parametrize("n", [65, 96, 97, 128])
def test_exact_families_workgroup(inv_wg, n, dtype):
    assert inv_wg.resolved_algo(n, 5) == g.ALGO_WORKGROUP
    a, x, names = _exact_batch(n, dtype, 2500)
    got, st = run(inv_wg, a)
    assert st == [OK] * len(names)
    for b, name in enumerate(names):
        assert canon(got[b]) == canon(x[b]), (n, name)


@DTYPES
def test_exact_families_one_ragged_call_over_all_orders(inv_wg, dtype):
    mats, want, tags = [], [], []
    for n in range(1, 129):
        for name, (a, x) in exact_families(n, 2600, dtype).items():
            mats.append(a)
            want.append(x)
            tags.append((n, name))
    order = np.random.default_rng(2600).permutation(len(mats))
    mats, want, tags = [mats[i] for i in order], [want[i] for i in order], [tags[i] for i in order]
    got, st = _run_strided(inv_wg, mats, dtype(-12345.5))
    assert st == [OK] * len(mats), [tags[b] for b, s in enumerate(st) if s][:8]
    for b in range(len(mats)):
        assert canon(got[b]) == canon(want[b]), tags[b]


# ---- 6. the overflow list --------------------------------------------------------------------------------------------
def _overflow_inputs(orders):
    return [(overflow(n, seed, mode, k), want, (n, seed, mode, k)) for n, seed, mode, k, want in OVERFLOW_LIST
            if n in orders]


@pytest.mark.parametrize("path", ["sweep", "blocked"])
def test_overflow_list_single_matrix_paths(oracle, inv_sweep, inv_blocked, path):
    inv = inv_sweep if path == "sweep" else inv_blocked
    cases = _overflow_inputs((8, 40, 100, 200))
    assert len(cases) == len(OVERFLOW_LIST)
    for a, listed, tag in cases:
        want, want_st = oracle_step(oracle, a)
        got, st = run(inv, a)
        assert st == [want_st] and want_st == listed, (tag, st, want_st)
        if want_st == OK:
            assert np.isfinite(got).all() and canonical_bytes(got) == canonical_bytes(want), tag


@pytest.mark.parametrize("path,n", [("resident", 8), ("resident", 40), ("workgroup", 100)])
def test_overflow_list_batched_paths(oracle, inv_resident, inv_wg, path, n):
    inv = inv_resident if path == "resident" else inv_wg
    cases = _overflow_inputs((n,))
    mats = np.stack([a for a, _, _ in cases])
    assert inv.resolved_algo(n, len(mats)) == (g.ALGO_RESIDENT if path == "resident" else g.ALGO_WORKGROUP)
    want = [oracle_step(oracle, a) for a in mats]
    assert [s for _, s in want] == [listed for _, listed, _ in cases] and len({s for _, s in want}) == 2
    got, st = run(inv, mats)
    assert st == [s for _, s in want], [t for _, _, t in cases]
    for b, (x, s) in enumerate(want):
        if s == OK:
            assert np.isfinite(got[b]).all() and canonical_bytes(got[b]) == canonical_bytes(x), cases[b][2]


# ---- 7. host entry points -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [40, 300])
def test_host_entry_points(n, monkeypatch):
    monkeypatch.delenv("MI32_SINGULAR_KEEP", raising=False)
    bad = [zero_column(n, n - 1, 2700 + n), zero_row(n, n // 2, 2701 + n)]
    for a in bad:
        assert g.matrix_inv_32(a.reshape(-1), n).size == 0
        assert g.matrix_inv_64(a.astype(np.float64).reshape(-1), n).size == 0
    mats = np.stack([gate_matrix(n, 2702 + n), bad[0], gate_matrix(n, 2703 + n), bad[1]])
    _, st = g.matrix_inv_32_batched(mats)
    assert st.tolist() == [OK, SINGULAR, OK, SINGULAR]
    for dtype, fn in ((np.float32, g.matrix_inv_32), (np.float64, g.matrix_inv_64)):
        for negz in (False, True):
            a, x = signed_pow2_permutation(n, 2704, dtype, negative_zeros=negz)
            got = fn(a.reshape(-1), n)
            assert got.dtype == dtype and got.size == n * n and canon(got) == canon(x), (dtype, negz)
    a, x = signed_pow2_permutation(n, 2705)
    out, st = g.matrix_inv_32_batched(np.stack([a, bad[0]]))
    assert st.tolist() == [OK, SINGULAR] and canonical_bytes(out[0]) == canonical_bytes(x)
    monkeypatch.setenv("MI32_SINGULAR_KEEP", "1")
    assert g.matrix_inv_32(bad[0].reshape(-1), n).size == n * n
    assert g.matrix_inv_64(bad[1].astype(np.float64).reshape(-1), n).size == n * n


# ---- 8. near-singular: duplicate rows -------------------------------------------------------------------------------
@pytest.mark.parametrize("path,n", [("sweep", 40), ("sweep", 100), ("sweep", 300), ("blocked", 40), ("blocked", 100),
                                    ("blocked", 300), ("resident", 8), ("resident", 40), ("workgroup", 100)])
def test_duplicate_rows_status_and_bits_as_the_oracle(oracle, inv_sweep, inv_blocked, inv_resident, inv_wg, path, n):
    inv = {"sweep": inv_sweep, "blocked": inv_blocked, "resident": inv_resident, "workgroup": inv_wg}[path]
    a = duplicate_rows(n, 2800 + n)
    want, want_st = oracle_step(oracle, a)
    aug, info = oracle.matrix_inv_32(a, n, return_info=True)
    assert want_st == info["status"] == OK and canonical_bytes(aug) == canonical_bytes(want)
    got, st = run(inv, a)
    assert st == [OK]
    assert canonical_bytes(got) == canonical_bytes(want), (path, n)
