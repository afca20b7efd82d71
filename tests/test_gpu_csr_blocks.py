"""GPU tests of the CSR block gather (``Inverter.csr_diag_blocks`` / ``inv_csr_blocks``, ``mi32_csr_blocks_device*``;
run with ``-m gpu`` on an MI355X): the diagonal blocks of a sparse matrix, orders 1 ... 128 mixed in one call, fp32 and
fp64 values, int32 and int64 indices.

There is no tolerance anywhere in this file: every comparison is bytes equal against the NumPy restatement by
assignment in tests/csr_cases.py (``mirror_blocks``), which tests/test_csr_cases.py holds to the dense matrix's blocks.
"""
import ctypes
import functools

import numpy as np
import pytest

import csr_cases as cc
from vbatch_cases import diag_block_orders

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_matrix_inversion_amd as g  # noqa: E402

VALUES = pytest.mark.parametrize("vdtype", [np.float32, np.float64], ids=["fp32", "fp64"])
INDICES = pytest.mark.parametrize("idtype", [np.int32, np.int64], ids=["int32", "int64"])


@pytest.fixture(scope="module")
def inv():
    i = g.Inverter()
    yield i
    i.close()


def _device(case, vdtype, idtype):
    """((crow, col, values) on the GPU, the host values) of a case."""
    crow, col, val = cc.typed(case, vdtype, idtype)
    return tuple(torch.from_numpy(x).cuda() for x in (crow, col, val)), val


def _gather(inverter, case, vdtype, idtype, **kw):
    """One csr_diag_blocks call; (the packed result on the host, the reference)."""
    dev, val = _device(case, vdtype, idtype)
    out = inverter.csr_diag_blocks(dev, case.orders, first_rows=case.first, **kw)
    torch.cuda.synchronize()
    assert out.dim() == 1 and out.dtype == dev[2].dtype and out.numel() == int((case.orders.astype(np.int64) ** 2).sum())
    want = cc.mirror_blocks(case.crow, case.col, val, case.orders, case.first, sources=getattr(case, "sources", None))
    return out.cpu().numpy(), want


# 1
@VALUES
@INDICES
def test_every_order_in_one_matrix(inv, vdtype, idtype):
    """Orders 1 ... 128 as the consecutive blocks of one matrix, through the ``torch.sparse_csr`` form of the argument."""
    case = cc.every_order_case()
    (crow, col, val), host = _device(case, vdtype, idtype)
    a = torch.sparse_csr_tensor(crow, col, val, size=(case.n, case.n))
    out = inv.csr_diag_blocks(a, case.orders)
    triple = inv.csr_diag_blocks((crow, col, val), case.orders)
    torch.cuda.synchronize()
    want = cc.mirror_blocks(case.crow, case.col, host, case.orders)
    cc.same_bytes(out.cpu().numpy(), want, "sparse_csr tensor")
    cc.same_bytes(triple.cpu().numpy(), want, "triple")


# 2
@VALUES
@INDICES
def test_seams(inv, vdtype, idtype):
    case = cc.seams_case()
    got, want = _gather(inv, case, vdtype, idtype)
    cc.same_bytes(got, want, "seams")
    # the inner entries, at the first and the last column of their block row, arrived; nothing else did
    stored = cc.typed(case, vdtype, idtype)[2]
    assert np.count_nonzero(got) == case.inner.size
    assert np.array_equal(np.sort(got[got != 0]), np.sort(stored[case.inner]))
    offs, _ = cc.flat_offsets(case.orders)
    for k, o in ((case.orders[0], offs[0]), (case.orders[-1], offs[-1])):         # the first and the last block
        blk = got[o:o + k * k].reshape(k, k)
        assert (blk[:, 0] != 0).all() and (blk[:, -1] != 0).all() and np.count_nonzero(blk) == (2 * k if k > 1 else 1)


# 3
@VALUES
@INDICES
def test_row_shapes(inv, vdtype, idtype):
    case = cc.row_shapes_case()
    got, want = _gather(inv, case, vdtype, idtype)
    cc.same_bytes(got, want, "row shapes")
    offs, _ = cc.flat_offsets(case.orders)
    dense = got[offs[6]:offs[6] + 128 * 128]
    assert (dense != 0).all()                                                     # the fully dense block of order 128
    for b in range(6):                                                            # the 700-entry rows brought every column
        k = int(case.orders[b])
        assert (got[offs[b] + k:offs[b] + 2 * k] != 0).all(), b


# 4
@VALUES
@INDICES
def test_values_arrive_bit_for_bit(inv, vdtype, idtype):
    case = cc.values_case()
    stored = cc.typed(case, vdtype, idtype)[2]
    size = stored.dtype.itemsize
    words = stored.view(cc.UINT[size])
    assert set(cc.special_bits(size).tolist()) <= set(words.tolist())             # the input holds them ...
    assert np.isnan(stored).any() and np.isinf(stored).any() and ((stored == 0) & np.signbit(stored)).any()
    assert ((np.abs(stored) > 0) & (np.abs(stored) < np.finfo(vdtype).tiny)).any()
    got, want = _gather(inv, case, vdtype, idtype)
    cc.same_bytes(got, want, "values")
    assert set(cc.special_bits(size).tolist()) <= set(got.view(cc.UINT[size]).tolist())   # ... and so does the output


# 5
@VALUES
@INDICES
def test_memory_contract_through_the_c_entry_point(inv, vdtype, idtype):
    """ldout = n + 3 with NaN in the padding, sentinel margins before and after every member, every member one element
    past a 256-byte boundary: the members equal the reference and no other byte of the buffer changes."""
    case = cc.seams_case()
    (crow, col, val), host = _device(case, vdtype, idtype)
    size = host.dtype.itemsize
    per_line = 256 // size
    orders = case.orders
    ld = orders + 3
    starts, at = [], 0
    for k, l in zip(orders, ld):
        at = (at + 8 + per_line - 1) // per_line * per_line + 1                   # at least 8 elements of margin
        starts.append(at)
        at += int(k) * int(l)
    total = at + 8
    sentinel, untouched = vdtype(-12345.5), vdtype(777.25)
    before = np.full(total, sentinel, vdtype)
    want = cc.mirror_blocks(case.crow, case.col, host, orders)
    offs, _ = cc.flat_offsets(orders)
    after = before.copy()
    for k, l, s, o in zip(orders, ld, starts, offs):
        k, l = int(k), int(l)
        for buf, member in ((before, untouched), (after, want[o:o + k * k].reshape(k, k))):
            region = buf[s:s + k * l].reshape(k, l)
            region[:, k:] = np.nan
            region[:, :k] = member
    tout = torch.from_numpy(before).cuda()
    assert tout.data_ptr() % 256 == 0
    ptrs = torch.from_numpy(np.asarray(starts, np.int64) * size + tout.data_ptr()).cuda()
    assert bool((ptrs % 256 == size).all())
    plan = inv.plan_ragged(orders)
    first = torch.from_numpy(cc.consecutive(orders)).cuda()
    tld = torch.from_numpy(ld.astype(np.int32)).cuda()
    inv._bind_stream()
    fn = inv._lib.mi32_csr_blocks_device if vdtype == np.float32 else inv._lib.mi32_csr_blocks_device_f64
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = fn(inv._h, plan._p, p(crow), p(col), np.dtype(idtype).itemsize, p(val), p(first), p(ptrs), p(tld))
    torch.cuda.synchronize()
    plan.close()
    assert rc == g.MI32_OK
    cc.same_bytes(tout.cpu().numpy(), after, "members, padding and margins")


# 6
@VALUES
@INDICES
def test_first_rows(inv, vdtype, idtype):
    case = cc.first_rows_case()
    got, want = _gather(inv, case, vdtype, idtype)
    cc.same_bytes(got, want, "overlapping blocks and gaps")


# 7
@VALUES
@INDICES
def test_many_small_members_in_one_launch_per_class(inv, vdtype, idtype):
    case = cc.many_members_case()
    dev, val = _device(case, vdtype, idtype)
    want = cc.mirror_blocks(case.crow, case.col, val, case.orders, sources=case.sources)
    inv.set_profiling(True)
    try:
        inv.get_profile()                                                         # drop what the call before left
        out = inv.csr_diag_blocks(dev, case.orders)
        launches = sum(count for _, count in inv.get_profile().values())
    finally:
        inv.set_profiling(False)
    torch.cuda.synchronize()
    classes = {cc.lanes_of(int(k)) for k in case.orders}
    assert launches <= 5 and launches == len(classes) == 1
    cc.same_bytes(out.cpu().numpy(), want, "70 000 members")


def test_launches_of_a_mixed_call(inv):
    case = cc.first_rows_case()
    dev, _ = _device(case, np.float32, np.int32)
    inv.set_profiling(True)
    try:
        inv.get_profile()
        inv.csr_diag_blocks(dev, case.orders, first_rows=case.first)
        prof = inv.get_profile()
    finally:
        inv.set_profiling(False)
    assert {k: c for k, (_, c) in prof.items() if c} == {"update_in_block": 5}      # the class of the apply launches


# 8
@functools.lru_cache(maxsize=None)
def _block_jacobi():
    orders = diag_block_orders()
    assert len(orders) == 43 and sum(orders) == 3000
    singular = next(b for b, k in enumerate(orders) if k > 8)
    return cc.block_jacobi_case(tuple(orders), singular=singular), singular


@VALUES
@INDICES
def test_end_to_end_against_the_dense_form(inv, vdtype, idtype):
    """The 43 diagonal blocks of a 3000-row matrix, one exactly singular: set-up from the CSR form against the set-up
    from the dense matrix, then both inverses applied."""
    case, singular = _block_jacobi()
    dev, _ = _device(case, vdtype, idtype)
    dense = torch.from_numpy(case.dense.astype(vdtype)).cuda()
    orders = case.orders
    x, st = inv.inv_csr_blocks(dev, orders)
    xd, std = inv.inv_diag_blocks(dense, orders, packed=True)
    x2, st2, (mant, exp) = inv.inv_csr_blocks(dev, orders, det=True)
    xd2, std2, (dmant, dexp) = inv.inv_diag_blocks(dense, orders, det=True, packed=True)
    torch.cuda.synchronize()
    sth = st.cpu().numpy()
    assert sth[singular] == g.MI32_SINGULAR and np.count_nonzero(sth) == 1
    assert np.array_equal(sth, std.cpu().numpy()) and np.array_equal(sth, st2.cpu().numpy())
    assert np.array_equal(sth, std2.cpu().numpy())
    cc.same_bytes(x.cpu().numpy(), xd.cpu().numpy(), "inverse")
    cc.same_bytes(x2.cpu().numpy(), xd2.cpu().numpy(), "inverse beside the determinant")
    cc.same_bytes(mant.cpu().numpy(), dmant.cpu().numpy(), "det mantissa")
    assert np.array_equal(exp.cpu().numpy(), dexp.cpu().numpy())
    r = torch.from_numpy(np.random.default_rng(81).uniform(-1, 1, (case.n, 2)).astype(vdtype)).cuda()
    z, zd = inv.apply_diag_blocks(x, orders, r), inv.apply_diag_blocks(xd, orders, r)
    torch.cuda.synchronize()
    cc.same_bytes(z.cpu().numpy(), zd.cpu().numpy(), "applied")


# 9
@VALUES
@INDICES
def test_stream_order(inv, vdtype, idtype):
    """Two calls with different matrices into the same ``out``, back to back, then one synchronise."""
    one, two = cc.every_order_case(), cc.every_order_case(7009)
    assert np.array_equal(one.orders, two.orders) and one.col.size != two.col.size
    dev1, _ = _device(one, vdtype, idtype)
    dev2, val2 = _device(two, vdtype, idtype)
    out = torch.full((int((one.orders.astype(np.int64) ** 2).sum()),), float("nan"), dtype=dev1[2].dtype, device="cuda")
    torch.cuda.synchronize()
    r1 = inv.csr_diag_blocks(dev1, one.orders, out=out)
    r2 = inv.csr_diag_blocks(dev2, two.orders, out=out)
    torch.cuda.synchronize()
    assert r1 is out and r2 is out
    cc.same_bytes(out.cpu().numpy(), cc.mirror_blocks(two.crow, two.col, val2, two.orders), "the second call's blocks")


def test_validate_and_refusals_on_a_live_inverter(inv):
    case = cc.seams_case()
    (crow, col, val), host = _device(case, np.float32, np.int64)
    out = inv.csr_diag_blocks((crow, col, val), case.orders, validate=True)
    torch.cuda.synchronize()
    cc.same_bytes(out.cpu().numpy(), cc.mirror_blocks(case.crow, case.col, host, case.orders), "validated")
    twice = col.clone()
    s = int(case.crow[np.argmax(np.diff(case.crow) >= 2)])
    twice[s + 1] = twice[s]
    bad = [lambda: inv.csr_diag_blocks((crow, twice, val), case.orders, validate=True),     # a pair stored twice
           lambda: inv.csr_diag_blocks((crow.cpu(), col.cpu(), val.cpu()), case.orders),    # not on the device
           lambda: inv.csr_diag_blocks((crow, col.int(), val), case.orders),                # two index dtypes
           lambda: inv.csr_diag_blocks((crow, col, val), case.orders[:-1]),                 # orders do not sum to N
           lambda: inv.csr_diag_blocks((crow, col, val), case.orders, first_rows=[0]),
           lambda: inv.csr_diag_blocks((crow, col, val), [100], first_rows=[case.n - 99]),  # leaves the matrix
           lambda: inv.csr_diag_blocks((crow, col, val), [129, case.n - 129]),              # an order above 128
           lambda: inv.csr_diag_blocks((crow, col, val), [4], out=val[:16], first_rows=[0]),  # out over values
           lambda: inv.csr_diag_blocks((crow, col, val), case.orders, out=torch.empty(3, device="cuda"))]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {i} was accepted")
