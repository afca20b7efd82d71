"""GPU tests of the block finder (``Inverter.csr_block_starts`` / ``csr_find_blocks``, ``mi32_csr_find_blocks_device``;
run with ``-m gpu`` on an MI355X): block-Jacobi blocks from a CSR sparsity pattern by supervariable agglomeration, int32
and int64 indices, ``max_order`` 1 ... 128, with and without agglomeration.

There is no tolerance anywhere in this file: every comparison is array equality against the NumPy restatement of the
definition in tests/find_blocks_cases.py (``mirror_starts``), which tests/test_find_blocks_cases.py holds to a
brute-force one.
"""
import numpy as np
import pytest

import find_blocks_cases as F

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_matrix_inversion_amd as g  # noqa: E402
from gpu_matrix_inversion_amd import api  # noqa: E402

INDICES = pytest.mark.parametrize("idtype", [np.int32, np.int64], ids=["int32", "int64"])
ORDERS = pytest.mark.parametrize("max_order", F.MAX_ORDERS)
FLAGS = pytest.mark.parametrize("agglomerate", [False, True], ids=["sv", "agglomerate"])


@pytest.fixture(scope="module")
def inv():
    i = g.Inverter()
    yield i
    i.close()


@pytest.fixture(scope="module")
def chunk():
    rows = api.find_blocks_chunk_rows()
    assert rows > 8 * 128
    return rows


def _device(case, idtype):
    crow, col = F.typed_pattern(case, idtype)
    return torch.from_numpy(crow).cuda(), torch.from_numpy(col).cuda()


def _same(got, want, tag):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == np.uint8 and got.shape == want.shape, (tag, got.dtype, got.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (tag, f"{bad.size} of {got.size} rows differ, first at {int(bad[0])}: "
                                f"{int(got[bad[0]])} for {int(want[bad[0]])}")


def _check(inverter, case, idtype, max_order, flags=(False, True), tag=""):
    crow, col = _device(case, idtype)
    for agglomerate in flags:
        got = inverter.csr_block_starts((crow, col, None), max_order, agglomerate=agglomerate)
        want = F.mirror_starts(case.crow, case.col, max_order, agglomerate, case.nat)
        _same(got, want, (tag, max_order, agglomerate))


# 1
@INDICES
@ORDERS
def test_edges(inv, idtype, max_order):
    """N = 1 and 2, and N at, one below and one above max_order: one run of N rows, and N rows that all differ."""
    for n in sorted({1, 2, max(1, max_order - 1), max_order, max_order + 1}):
        _check(inv, F.common_pattern_case(n), idtype, max_order, tag=("common", n))
        _check(inv, F.tridiagonal_case(n), idtype, max_order, tag=("tridiagonal", n))
    _check(inv, F.from_rows([[0, 1], [0, 1]]), idtype, max_order, tag="two equal rows")
    _check(inv, F.from_rows([[], []]), idtype, max_order, tag="two empty rows")
    _check(inv, F.from_rows([[]]), idtype, max_order, tag="one empty row")


# 2
@INDICES
def test_rows_that_differ_in_one_entry(inv, idtype):
    """The first, a middle and the last entry; one entry more; 700 entries of which the last differs; empty rows; the
    same set in another stored order."""
    case = F.one_entry_case()
    crow, col = _device(case, idtype)
    got = inv.csr_block_starts((crow, col, None), 128, agglomerate=False).cpu().numpy()
    # with max_order 128 and no agglomeration the starts are the natural boundaries wherever runs are short
    for row, nat in case.want_nat.items():
        assert got[row] == nat, (row, nat)
    for max_order in (1, 2, 8, 32, 128):
        _check(inv, case, idtype, max_order, tag="one entry")


# 3
@INDICES
@ORDERS
def test_run_lengths(inv, idtype, max_order):
    n = 1001 if max_order > 1 else 301
    assert n % max_order != 0 or max_order == 1
    common, tri = F.common_pattern_case(n), F.tridiagonal_case(n)
    _check(inv, common, idtype, max_order, tag="one run")
    _check(inv, tri, idtype, max_order, tag="tridiagonal")
    crow, col = _device(common, idtype)
    full = [max_order] * (n // max_order) + ([n % max_order] if n % max_order else [])
    for agglomerate in (False, True):       # one run of N, cut every max_order: full supervariables do not merge
        assert inv.csr_find_blocks((crow, col, None), max_order, agglomerate=agglomerate).tolist() == full
    crow, col = _device(tri, idtype)        # single rows: every block is full but the last
    assert inv.csr_find_blocks((crow, col, None), max_order, agglomerate=False).tolist() == [1] * n
    assert inv.csr_find_blocks((crow, col, None), max_order).tolist() == full


# 4
@INDICES
@ORDERS
@pytest.mark.parametrize("kind", F.SEAM_KINDS)
def test_chunk_seams(inv, chunk, idtype, max_order, kind):
    """Over each of the first three seams between chunks: a natural run longer than max_order, a block that starts
    max_order - 1 rows before the seam, a supervariable boundary exactly on it; N = three chunks and a prime."""
    case = F.seams_case(chunk, max_order, kind)
    assert case.n == 3 * chunk + 293
    _check(inv, case, idtype, max_order, tag=kind)


# 5
@INDICES
@pytest.mark.parametrize("dof,grid", [(3, (10, 9, 8)), (5, (6, 6, 5))])
def test_node_blocks(inv, idtype, dof, grid):
    case = F.stencil27_case(grid, dof)
    assert case.n % 30 == 0
    crow, col = _device(case, idtype)
    assert set(inv.csr_find_blocks((crow, col, None), 32, agglomerate=False).tolist()) == {dof}
    assert set(inv.csr_find_blocks((crow, col, None), 32).tolist()) == {30}
    for max_order in (1, 2, 8, 32, 127, 128):
        _check(inv, case, idtype, max_order, tag=("stencil", dof))


# 6
@INDICES
@FLAGS
@pytest.mark.parametrize("max_order", [8, 32, 128])
def test_long_chain(inv, chunk, idtype, agglomerate, max_order):
    """64 chunks of rows in runs of 1 ... 200: the chain over the chunks and the two-level run start, at length."""
    case = F.long_chain_case(chunk)
    assert case.n >= 64 * chunk
    crow, col = _device(case, idtype)
    got = inv.csr_block_starts((crow, col, None), max_order, agglomerate=agglomerate)
    _same(got, F.long_chain_want(chunk, max_order, agglomerate), ("long chain", max_order, agglomerate))


# 7
@INDICES
def test_forms_and_repeat_calls(inv, chunk, idtype):
    case = F.seams_case(chunk, 32, "run")
    crow, col = _device(case, idtype)
    want = {(m, a): F.mirror_starts(case.crow, case.col, m, a, case.nat) for m in (8, 32) for a in (False, True)}
    # the torch.sparse_csr form against the triple form (the runs' columns are sorted, as torch wants them)
    sp = torch.sparse_csr_tensor(crow, col, torch.ones(col.numel(), device="cuda"), size=(case.n, case.n))
    _same(inv.csr_block_starts(sp, 32), want[32, True], "sparse_csr")
    _same(inv.csr_block_starts((crow, col, sp.values()), 32), want[32, True], "triple with values")
    _same(inv.csr_block_starts((crow, col, None)), want[32, True], "defaults")
    assert np.array_equal(inv.csr_find_blocks(sp), F.orders_of(want[32, True]))
    assert inv.csr_find_blocks(sp).dtype == np.int32
    # out= reuse: the same tensor comes back, and every element is written by every call
    out = torch.full((case.n,), 7, dtype=torch.uint8, device="cuda")
    for key in ((8, False), (32, True), (8, True)):
        assert inv.csr_block_starts((crow, col, None), key[0], agglomerate=key[1], out=out) is out
        _same(out, want[key], ("out", key))
    # two calls back to back on one context, different max_order, different outputs, no host synchronisation between
    a, b = torch.full_like(out, 9), torch.full_like(out, 9)
    inv.csr_block_starts((crow, col, None), 8, out=a)
    inv.csr_block_starts((crow, col, None), 32, agglomerate=False, out=b)
    inv.csr_block_starts((crow, col, None), 32, out=out)
    torch.cuda.synchronize()
    _same(a, want[8, True], "first of three")
    _same(b, want[32, False], "second of three")
    _same(out, want[32, True], "third of three")
    # a wrong argument is a ValueError
    with pytest.raises(ValueError):
        inv.csr_block_starts((crow, col, None), 129)
    with pytest.raises(ValueError):
        inv.csr_block_starts((crow, col, None), 32, out=out[:-1])
    with pytest.raises(ValueError):
        inv.csr_block_starts((crow.cpu(), col.cpu(), None), 32)


# 8
def test_end_to_end_block_jacobi(inv):
    """From a bare CSR matrix: the orders found on the device drive ``inv_csr_blocks`` and ``apply_diag_blocks`` to
    the bytes the mirror's orders give."""
    case = F.block_jacobi_case([5, 12, 32, 7, 20, 1, 64, 3, 16, 9])
    crow, col, val = (torch.from_numpy(x).cuda() for x in F.typed(case, np.float32, np.int64))
    orders = inv.csr_find_blocks((crow, col, val), 32)
    want = F.orders_of(F.mirror_starts(case.crow, case.col, 32, True))
    assert np.array_equal(orders, want) and orders.dtype == np.int32
    assert int(orders.sum()) == case.n and orders.min() >= 1 and orders.max() <= 32
    r = torch.from_numpy(np.random.default_rng(7500).uniform(-1, 1, (case.n, 3)).astype(np.float32)).cuda()
    results = []
    for o in (orders, want):
        x, status = inv.inv_csr_blocks((crow, col, val), o)
        z = inv.apply_diag_blocks(x, o, r)
        torch.cuda.synchronize()
        results.append((x.cpu().numpy(), status.cpu().numpy(), z.cpu().numpy()))
    for got, ref in zip(*results):
        assert got.tobytes() == ref.tobytes()
