"""GPU tests of the block residual and the fused block-Jacobi sweep (``Inverter.csr_block_residual`` /
``Inverter.relax_stored``, ``mi32_csr_block_residual_device*`` / ``mi32_csr_relax_stored_device*`` of
include/mat_inv_32_relax.h; run with ``-m gpu`` on an MI355X).

There is no tolerance in this file.  The residual has the bits of tests/relax_mirror.c; x' has the bits of the sweep
mirror (that residual, tests/apply_mirror.c on the NumPy-widened members, one fma) and of the same sweep composed from
this library's own calls; a NaN stands exactly where the expectation has one (``apply_cases.assert_same_bits``).
fp32 and fp64, int32 and int64 indices."""
import functools

import numpy as np
import pytest

import relax_cases as rc
import stored_cases as sc
from apply_cases import assert_same_bits, bits, build_apply_mirror
from vbatch_cases import pack, unpack

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_matrix_inversion_amd as g  # noqa: E402

DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
INDEX = pytest.mark.parametrize("index", [np.int32, np.int64], ids=["int32", "int64"])
SEAMS = (0, 1, 7, 8, 9, 15, 16, 17)


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return rc.build_relax_mirror(tmp_path_factory.mktemp("relax_mirror"))


@pytest.fixture(scope="module")
def adll(tmp_path_factory):
    return build_apply_mirror(tmp_path_factory.mktemp("apply_mirror"))


@pytest.fixture(scope="module")
def inv():
    i = g.Inverter()
    yield i
    i.close()


def dev(a, dt=None):
    a = np.asarray(a)
    return torch.from_numpy(a if dt is None else a.astype(dt)).cuda()


def dev_csr(csr, index):
    return dev(csr[0], index), dev(csr[1], index), dev(csr[2])


def vectors(n, seed, dtype):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, n).astype(dtype), rng.uniform(-1, 1, n).astype(dtype)


def store_of(inv, members, formats):
    """(plan, stored, widened members) of members stored in the given formats."""
    orders, flat = pack(members)
    plan = inv.plan_ragged(orders)
    stored = inv.store_inverses(plan, dev(flat), np.asarray(formats, np.int32))
    return plan, stored, [sc.roundtrip(m, int(f)) for m, f in zip(members, formats)]


def check_calls(dll, adll, inv, csr, index, plan, stored, wide, first, x, b, omega, tag, first_rows=None):
    """The three statements of the every-order test on one input: residual = mirror, sweep = sweep mirror, sweep = the
    library's own residual and apply_stored, then one exact fma."""
    a = dev_csr(csr, index)
    rows = rc.block_rows(first, plan.orders)
    r = inv.csr_block_residual(a, plan, dev(x), dev(b), first_rows=first_rows)
    xn = inv.relax_stored(a, stored, dev(x), dev(b), omega, first_rows=first_rows)
    z = inv.apply_stored(stored, r)
    torch.cuda.synchronize()
    r, xn, z = r.cpu().numpy(), xn.cpu().numpy(), z.cpu().numpy()
    assert_same_bits(r, rc.mirror_residual(dll, csr, x, b, rows), (tag, "residual"))
    assert_same_bits(xn, rc.mirror_sweep(dll, adll, csr, first, wide, x, b, omega), (tag, "sweep"))
    composed = x.copy()
    composed[rows] = rc.mirror_axpy(dll, omega, z, x[rows])
    assert_same_bits(xn, composed, (tag, "composed"))
    return xn


# ---- every order in one matrix ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _every_order(dtype):
    """(csr, orders, first, members, formats): every order 1 ... 128 once, shuffled, N = 8256; rows of 0 ... 40 entries
    and one of 700, columns in drawn (unsorted) order; members inside float16's normal range in cycling formats."""
    orders = np.random.default_rng(31).permutation(np.arange(1, 129))
    n = int(orders.sum())
    lengths = np.random.default_rng(32).integers(0, 41, n)
    lengths[4321] = 700
    csr = rc.random_rows(n, lengths, 33, dtype)
    return csr, orders, rc.first_of(orders), sc.members_in_range(orders, 34, dtype), sc.cycling_formats(orders, dtype)


@DTYPES
@INDEX
def test_every_order_in_one_matrix(dll, adll, inv, dtype, index):
    csr, orders, first, members, formats = _every_order(dtype)
    assert csr[0].size - 1 == 8256 and sorted(orders) == list(range(1, 129))
    assert set(np.diff(csr[0]).tolist()) >= set(range(41)) | {700}
    plan, stored, wide = store_of(inv, members, formats)
    x, b = vectors(8256, 35, dtype)
    check_calls(dll, adll, inv, csr, index, plan, stored, wide, first, x, b, 0.75, "every order")
    plan.close()


# ---- row lengths at the eight-lane seams -----------------------------------------------------------------------------
@DTYPES
@INDEX
def test_row_lengths_at_the_eight_lane_seams(dll, adll, inv, dtype, index):
    """Orders 3, 12, 24, 48 and 100, one per lane class (three of order 3, so that they hold every length too); the
    rows of every member cycle through the lengths 0, 1, 7, 8, 9, 15, 16, 17."""
    orders = np.array([3, 3, 3, 12, 24, 48, 100])
    n = int(orders.sum())
    lengths = [SEAMS[i % len(SEAMS)] for i in range(n)]
    csr = rc.random_rows(n, lengths, 41, dtype)
    first = rc.first_of(orders)
    for f, m in zip(first[2:], orders[2:]):
        assert set(lengths[f:f + m]) == set(SEAMS) or m == 3
    plan, stored, wide = store_of(inv, sc.members_in_range(orders, 42, dtype), sc.cycling_formats(orders, dtype))
    x, b = vectors(n, 43, dtype)
    check_calls(dll, adll, inv, csr, index, plan, stored, wide, first, x, b, 1.0, "seams")
    plan.close()


# ---- store formats ---------------------------------------------------------------------------------------------------
@DTYPES
def test_mixed_store_of_the_adaptive_setup(dll, adll, inv, dtype):
    """``inv_csr_blocks_adaptive`` on the row-scaled convergence matrix chooses at least two formats; the sweep follows
    the mirror on the members decoded from the store's own bytes."""
    csr, orders, first = rc.scaled_jacobi_matrix(dtype)
    a = dev_csr(csr, np.int32)
    stored, status, formats = inv.inv_csr_blocks_adaptive(a, orders)
    torch.cuda.synchronize()
    formats = formats.cpu().numpy()
    assert (status.cpu().numpy() == 0).all() and len(set(formats.tolist())) >= 2, np.bincount(formats, minlength=4)
    wide = rc.decode_store(stored.data.cpu().numpy(), orders, formats, dtype)
    x, b = vectors(csr[0].size - 1, 51, dtype)
    check_calls(dll, adll, inv, csr, np.int32, stored.plan, stored, wide, first, x, b, 1.0, "adaptive")
    stored.plan.close()


@functools.lru_cache(maxsize=None)
def _jacobi(dtype):
    csr, orders, first = rc.jacobi_matrix(dtype)
    return csr, orders, first, rc.block_inverses(csr, orders, first, dtype)


@DTYPES
@pytest.mark.parametrize("code", [sc.FLOAT16, sc.BFLOAT16, sc.NATIVE], ids=["float16", "bfloat16", "native"])
def test_stores_forced_to_one_format(dll, adll, inv, dtype, code):
    csr, orders, first, xs = _jacobi(dtype)
    plan, stored, wide = store_of(inv, xs, [code] * len(orders))
    x, b = vectors(csr[0].size - 1, 52, dtype)
    check_calls(dll, adll, inv, csr, np.int64, plan, stored, wide, first, x, b, 0.875, ("forced", code))
    plan.close()


# ---- start from zero -------------------------------------------------------------------------------------------------
@DTYPES
def test_from_zero_the_sweep_is_the_apply(inv, dtype):
    """x = 0, omega = 1: every product of the residual is a zero, r = b, and x' = fma(1, z, 0) has the bits of
    ``apply_stored(stored, b)`` (consecutive blocks: the packed layout is the row order)."""
    csr, orders, first, xs = _jacobi(dtype)
    plan, stored, _ = store_of(inv, xs, [sc.FLOAT16] * len(orders))
    n = csr[0].size - 1
    b = vectors(n, 53, dtype)[1]
    xn = inv.relax_stored(dev_csr(csr, np.int32), stored, dev(np.zeros(n, dtype)), dev(b))
    z = inv.apply_stored(stored, dev(b))
    torch.cuda.synchronize()
    plan.close()
    assert_same_bits(xn.cpu().numpy(), z.cpu().numpy(), "from zero")


# ---- stored order defines the bits -----------------------------------------------------------------------------------
@DTYPES
def test_stored_order_defines_the_bits(dll, adll, inv, dtype):
    """The same rows with their columns as drawn and sorted ascending: each follows the mirror in its own stored order,
    and the two differ."""
    orders = np.array([5, 14, 30, 60, 90])
    n = int(orders.sum())
    lengths = np.random.default_rng(61).integers(20, 41, n)
    first = rc.first_of(orders)
    plan, stored, wide = store_of(inv, sc.members_in_range(orders, 62, dtype), [sc.NATIVE] * len(orders))
    x, b = vectors(n, 63, dtype)
    got = []
    for sort in (False, True):
        csr = rc.random_rows(n, lengths, 64, dtype, sort=sort)
        assert (np.diff(csr[1][csr[0][3]:csr[0][4]]) > 0).all() == sort
        got.append(check_calls(dll, adll, inv, csr, np.int32, plan, stored, wide, first, x, b, 1.0, ("sorted", sort)))
    plan.close()
    assert (bits(got[0]) != bits(got[1])).any()


# ---- gaps and margins ------------------------------------------------------------------------------------------------
@DTYPES
@INDEX
def test_gaps_margins_and_untouched_inputs(dll, adll, inv, dtype, index):
    """Blocks that skip rows, given out of order; ``out`` pre-filled with a NaN of a payload of its own: covered rows
    get the mirror's bits, every other row keeps the sentinel's, and nothing the call reads changes by a byte."""
    orders = np.array([40, 5, 70, 17, 3])
    first = np.array([40, 2, 90, 10, 180])
    n = 200
    csr = rc.random_rows(n, np.random.default_rng(71).integers(0, 30, n), 72, dtype)
    plan, stored, wide = store_of(inv, sc.members_in_range(orders, 73, dtype), sc.cycling_formats(orders, dtype))
    x, b = vectors(n, 74, dtype)
    a, dx, db = dev_csr(csr, index), dev(x), dev(b)
    before = [t.cpu().numpy().copy() for t in (*a, dx, db, stored.data)]
    word = np.uint32 if dtype == np.float32 else np.uint64
    sentinel = np.array([0x7FC12345 if dtype == np.float32 else 0x7FF8000012345678], word).view(dtype)[0]
    out = dev(np.full(n, sentinel, dtype))
    got = inv.relax_stored(a, stored, dx, db, 0.5, out=out, first_rows=first)
    fresh = inv.relax_stored(a, stored, dx, db, 0.5, first_rows=first)
    twice = inv.relax_stored(a, stored, dx, db, 0.5, first_rows=first, sweeps=2)
    torch.cuda.synchronize()
    assert got is out
    rows = rc.block_rows(first, orders)
    covered = np.zeros(n, bool)
    covered[rows] = True
    assert not covered.all()
    want = rc.mirror_sweep(dll, adll, csr, first, wide, x, b, 0.5)
    got = got.cpu().numpy()
    assert_same_bits(got[covered], want[covered], "covered rows")
    assert (bits(got[~covered]) == bits(np.full(n, sentinel, dtype))[~covered]).all()
    assert_same_bits(fresh.cpu().numpy(), want, "out=None keeps x in the rows of no block")
    assert_same_bits(twice.cpu().numpy(), rc.mirror_sweep(dll, adll, csr, first, wide, x, b, 0.5, sweeps=2), "two sweeps, gaps")
    for t, was in zip((*a, dx, db, stored.data), before):
        assert t.cpu().numpy().tobytes() == was.tobytes()
    # overlapping blocks are the residual call's business still
    lap = np.array([0, 38, 60, 100, 102])
    r = inv.csr_block_residual(a, plan, dx, db, first_rows=lap)
    torch.cuda.synchronize()
    plan.close()
    assert_same_bits(r.cpu().numpy(), rc.mirror_residual(dll, csr, x, b, rc.block_rows(lap, orders)), "overlapping residual")


# ---- many members ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,index", [(np.float32, np.int32), (np.float64, np.int64)], ids=["fp32-int32", "fp64-int64"])
def test_many_members_in_one_call(dll, adll, inv, dtype, index):
    orders = np.random.default_rng(81).integers(1, 4, 70000)
    n = int(orders.sum())
    csr = rc.random_rows_fast(n, np.random.default_rng(82).integers(0, 6, n), 83, dtype)
    first = rc.first_of(orders)
    # the members drawn, stored and widened as ONE packed array (member by member would take the test's time)
    rng = np.random.default_rng(84)
    size = int((orders.astype(np.int64) ** 2).sum())
    flat = (rng.choice([-1.0, 1.0], size) * 2.0 ** rng.uniform(-12, 12, size)).astype(dtype)
    formats = np.array(sc.codes_of(dtype), np.int32)[np.arange(orders.size) % len(sc.codes_of(dtype))]
    per_element = np.repeat(formats, orders.astype(np.int64) ** 2)
    wide_flat = flat.copy()
    for code in sc.codes_of(dtype):
        wide_flat[per_element == code] = sc.roundtrip(flat[per_element == code], code)
    wide = unpack(wide_flat, orders)
    plan = inv.plan_ragged(orders)
    stored = inv.store_inverses(plan, dev(flat), formats)
    x, b = vectors(n, 85, dtype)
    xn = inv.relax_stored(dev_csr(csr, index), stored, dev(x), dev(b), 1.0)
    torch.cuda.synchronize()
    plan.close()
    assert_same_bits(xn.cpu().numpy(), rc.mirror_sweep(dll, adll, csr, first, wide, x, b, 1.0), "70 000 members")


# ---- repeated sweeps -------------------------------------------------------------------------------------------------
@DTYPES
def test_six_sweeps_in_one_call(dll, adll, inv, dtype):
    """``sweeps=6`` from x = 0 on the convergence matrix against six mirror sweeps: the bytes carry the convergence that
    tests/test_relax_mirror.py holds the mirror to."""
    csr, orders, first, xs = _jacobi(dtype)
    plan, stored, wide = store_of(inv, xs, [sc.NATIVE] * len(orders))
    n = csr[0].size - 1
    b = vectors(n, 91, dtype)[1]
    x = np.zeros(n, dtype)
    a = dev_csr(csr, np.int32)
    out = dev(np.full(n, np.nan, dtype))
    got = inv.relax_stored(a, stored, dev(x), dev(b), sweeps=6, out=out)
    odd = inv.relax_stored(a, stored, dev(x), dev(b), sweeps=5)
    torch.cuda.synchronize()
    plan.close()
    assert got is out
    assert_same_bits(got.cpu().numpy(), rc.mirror_sweep(dll, adll, csr, first, wide, x, b, sweeps=6), "six sweeps")
    assert_same_bits(odd.cpu().numpy(), rc.mirror_sweep(dll, adll, csr, first, wide, x, b, sweeps=5), "five sweeps")
