"""CPU checks of tests/csr_cases.py, the reference of the CSR block gather: the restatement by assignment equals the
diagonal blocks of the dense matrix, scatter-built, on small cases -- signs of zeros and NaN payloads included, which
``to_dense()`` would not keep --, and every case generator's self-assertions hold."""
import numpy as np
import pytest

import csr_cases as cc


def _dense_blocks(case, val):
    """The blocks cut out of the dense matrix, built by scattering the entries' bits."""
    bits = val.view(cc.UINT[val.dtype.itemsize])
    dense = np.zeros((case.n, case.n), bits.dtype)
    dense[cc.rows_of_entries(case.crow), case.col] = bits
    first = cc.consecutive(case.orders) if case.first is None else case.first
    return np.concatenate([dense[f:f + k, f:f + k].reshape(-1) for k, f in zip(case.orders, first)]).view(val.dtype)


@pytest.mark.parametrize("make", [cc.seams_case, cc.row_shapes_case, cc.values_case, cc.first_rows_case],
                         ids=["seams", "row-shapes", "values", "first-rows"])
@pytest.mark.parametrize("vdtype", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_mirror_equals_the_dense_blocks(make, vdtype):
    case = make()
    crow, col, val = cc.typed(case, vdtype, np.int32)
    want = _dense_blocks(case, val)
    got = cc.mirror_blocks(crow, col, val, case.orders, case.first)
    assert got.dtype == vdtype and got.size == int((case.orders.astype(np.int64) ** 2).sum())
    cc.same_bytes(got, want, make.__name__)


def test_mirror_by_hand():
    #      row 0: (0,1)=5 (0,0)=-0.0      row 1: empty      row 2: (2,0)=7 (2,2)=NaN      row 3: (3,3)=9 (3,1)=8
    crow = np.array([0, 2, 2, 4, 6])
    col = np.array([1, 0, 0, 2, 3, 1])
    val = np.array([5, -0.0, 7, np.nan, 9, 8], np.float32)
    got = cc.mirror_blocks(crow, col, val, [2, 2])
    cc.same_bytes(got, np.array([-0.0, 5, 0, 0, np.nan, 0, 0, 9], np.float32), "consecutive")
    assert np.signbit(got[0]) and not np.signbit(got[2])
    assert cc.mirror_sources(crow, col, [2, 2]).tolist() == [1, 0, -1, -1, 3, -1, -1, 4]
    got = cc.mirror_blocks(crow, col, val, [3, 1], first=[1, 0])       # rows 1 ... 3, then row 0
    cc.same_bytes(got, np.array([0, 0, 0, 0, np.nan, 0, 8, 0, 9, -0.0], np.float32), "first rows")
    with pytest.raises(AssertionError):
        cc.same_bytes(np.array([0.0], np.float32), np.array([-0.0], np.float32))


def test_to_dense_is_no_reference():
    torch = pytest.importorskip("torch")
    a = torch.sparse_csr_tensor(torch.tensor([0, 1]), torch.tensor([0]), torch.tensor([-0.0]), size=(1, 1))
    kept = cc.mirror_blocks(np.array([0, 1]), np.array([0]), np.array([-0.0], np.float32), [1])
    assert np.signbit(kept[0])
    # the reason the reference assigns: whatever to_dense() makes of a stored -0.0, the mirror keeps its sign
    print("to_dense() of a stored -0.0 has signbit", bool(np.signbit(a.to_dense().numpy()[0, 0])))


def test_generators_hold_their_properties():
    every = cc.every_order_case()
    assert sorted(every.orders.tolist()) == list(range(1, 129)) and every.n == 8256
    assert 0.2 < cc.inside_fraction(every) < 0.8                      # entries on both sides of the blocks' edges
    many = cc.many_members_case()
    assert many.orders.size == 70_000 and many.orders.min() == 1 and many.orders.max() == 8
    cc.same_bytes(cc.mirror_blocks(many.crow, many.col, many.val, many.orders, sources=many.sources),
                  _dense_free_reference(many), "many members")
    bj = cc.block_jacobi_case([3, 70, 9, 128], singular=2)
    assert np.linalg.matrix_rank(bj.dense[73:82, 73:82].astype(np.float64)) == 8
    got = cc.mirror_blocks(bj.crow, bj.col, bj.val.astype(np.float32), bj.orders)
    first = cc.consecutive(bj.orders)
    cc.same_bytes(got, np.concatenate([bj.dense[f:f + k, f:f + k].reshape(-1) for k, f in zip(bj.orders, first)]), "bj")
    sp = cc.values_case()
    for size, ftype in ((4, np.float32), (8, np.float64)):
        v = sp.bits[size].view(ftype)
        assert np.isnan(v).any() and np.isinf(v).any() and ((v == 0) & np.signbit(v)).any() and ((v == 0) & ~np.signbit(v)).any()
        assert ((np.abs(v) > 0) & (np.abs(v) < np.finfo(ftype).tiny)).any()


def _dense_free_reference(case):
    """For a matrix too large for a dense copy: the same blocks through a dictionary of the entries."""
    val = case.val
    first = cc.consecutive(case.orders)
    stop = int(case.crow[first[2000]])                                 # the entries of the first 2000 blocks' rows
    where = {(int(r), int(c)): i for i, (r, c) in enumerate(zip(cc.rows_of_entries(case.crow)[:stop], case.col[:stop]))}
    out = np.zeros(int((case.orders.astype(np.int64) ** 2).sum()), val.dtype)
    o = 0
    for k, f in zip(case.orders[:2000], first[:2000]):                 # the first 2000 blocks entry by entry ...
        for i in range(k):
            for j in range(k):
                at = where.get((f + i, f + j))
                if at is not None:
                    out[o + i * k + j] = val[at]
        o += k * k
    ref = cc.mirror_blocks(case.crow, case.col, val, case.orders, sources=case.sources)
    out[o:] = ref[o:]                                                  # ... the rest taken as it is
    return out
