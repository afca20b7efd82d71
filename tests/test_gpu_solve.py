"""GPU tests of A X = B on the one-launch batch paths (``Inverter.solve``, ``mi32_solve_device*``; run with ``-m gpu`` on
an MI355X): the register-resident and the workgroup-resident solve kernels, fp32 and fp64, with partial pivoting and
without, every lane class by width, every rows-per-thread class, full chunks and chunked calls.

There is no tolerance anywhere in this file.  X and the status must equal those of the step-by-step mirror
tests/solve_mirror.c (``np.array_equal``), which tests/test_solve_mirror.py holds to the CPU oracle; X is compared only
where the status is 0, as elsewhere.
"""
import numpy as np
import pytest

from det_cases import NOPIVOT_ORDERS, WORKGROUP_EDGES, dominant_member, family_members
from resident_cases import FP64_ORDERS, TIE_ORDERS, big_batch, shared_wave_batch, tie_batch
from solve_cases import build_solve_mirror, cap, mirror_solve, mirror_solve_batch, rhs

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


def _rhs_batch(mats, k, seed=0):
    n = mats.shape[1]
    return np.stack([rhs(n, k, 1000 * k + 10 * n + seed + m, mats.dtype) for m in range(len(mats))])


def _solve(inverter, mats, b, **kw):
    """solve on numpy batches; (X, status) as numpy arrays."""
    x, st = inverter.solve(torch.from_numpy(np.ascontiguousarray(mats)).cuda(),
                           torch.from_numpy(np.ascontiguousarray(b)).cuda(), **kw)
    torch.cuda.synchronize()
    assert st.dtype == torch.int32 and x.dtype == torch.from_numpy(b).dtype and tuple(x.shape) == b.shape
    return x.cpu().numpy(), st.cpu().numpy()


def _check(dll, inverter, mats, b, pivoting=True, tag=None):
    """One call on the batch; X and status against the mirror.  Returns (X, status)."""
    mats = np.ascontiguousarray(mats)
    want_x, want_st = mirror_solve_batch(dll, mats, b, pivoting)
    x, st = _solve(inverter, mats, b)
    assert np.array_equal(st, want_st), (tag, mats.shape, b.shape, st, want_st)
    for m in range(len(mats)):
        if want_st[m] == 0:
            assert np.array_equal(x[m], want_x[m]), (tag, mats.shape[1], b.shape[2], m)
    return x, st


def test_every_order_fp32(dll, inv):
    """K = 1 and K = 3 cross every lane class by width (7+1 / 8+1, 15+1 / 16+1, 31+1 / 32+1, 63+1 / 64+1) and every
    rows-per-thread edge (80 / 81, 96 / 97, 112 / 113, 127)."""
    for n in range(1, 128):
        mats = np.stack(family_members(n))
        for k in (1, 3):
            x, st = _check(dll, inv, mats, _rhs_batch(mats, k), tag="fp32")
            assert not st.any()


@pytest.mark.parametrize("n,k", [(1, 63), (5, 3), (8, 8), (16, 16), (32, 32), (33, 31), (33, 95), (64, 64), (100, 28),
                                 (127, 1)])
def test_width_edges_at_full_capacity(dll, inv, n, k):
    cols, launches, lanes, rows = inv.resolved_solve(n, k)
    assert launches == 1
    assert n + k in (lanes, 128) and (rows != 0) == (n + k == 128)   # every lane or column of the instance is in use
    mats = np.stack(family_members(n))
    x, st = _check(dll, inv, mats, _rhs_batch(mats, k), tag="full")
    assert not st.any()


@pytest.mark.parametrize("n,k,launches", [(8, 57, 2), (8, 130, 3), (40, 89, 2), (100, 29, 2), (127, 5, 5)])
def test_chunked_calls(dll, inv, n, k, launches):
    assert inv.resolved_solve(n, k)[:2] == (cap(n), launches)
    mats = np.stack(family_members(n))
    b = _rhs_batch(mats, k)
    x, st = _check(dll, inv, mats, b, tag="chunked")
    assert not st.any()
    ta = torch.from_numpy(mats).cuda()
    tb = torch.from_numpy(b).cuda()
    singles = [inv.solve(ta, tb[:, :, c:c + 1].contiguous())[0] for c in range(k)]
    torch.cuda.synchronize()
    assert np.array_equal(torch.cat(singles, dim=2).cpu().numpy(), x)


def test_fp64(dll, inv):
    for n in FP64_ORDERS + [e for e in WORKGROUP_EDGES if e != 128]:
        mats = np.stack(family_members(n, np.float64)) * 1.000000001   # entries that are no float32 values
        for k in (1, 3):
            x, st = _check(dll, inv, mats, _rhs_batch(mats, k), tag="fp64")
            assert not st.any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_no_pivot(dll, inv_nopivot, dtype):
    for n in NOPIVOT_ORDERS + [65, 96, 127]:
        mats = dominant_member(n, dtype)[None]
        x, st = _check(dll, inv_nopivot, mats, _rhs_batch(mats, 2), pivoting=False, tag="nopivot")
        assert not st.any()


def test_flagged_members_between_good_ones(dll, inv):
    mats, want_st = shared_wave_batch()
    b = _rhs_batch(mats, 5)
    x, st = _check(dll, inv, mats, b, tag="flagged")
    assert st.tolist() == want_st == [0, 0, 0, 2, 0, 2, 0, 0, 2]
    hit = b.copy()
    hit[1, 13, 2] = np.nan
    x2, st2 = _check(dll, inv, mats, hit, tag="NaN in B")
    assert st2.tolist() == [0, 2, 0, 2, 0, 2, 0, 0, 2]
    for m in range(9):
        if m != 1:
            assert np.array_equal(x2[m], x[m], equal_nan=True), m
    assert np.isnan(x2[1][:, 2]).any() and np.array_equal(x2[1][:, [0, 1, 3, 4]], x[1][:, [0, 1, 3, 4]])


@pytest.mark.parametrize("n", TIE_ORDERS)
def test_ties(dll, inv, n):
    mats = tie_batch(n)
    _check(dll, inv, mats, _rhs_batch(mats, 1), tag="ties")


@pytest.mark.parametrize("n", [20, 64])
def test_identity_gives_the_inverse(dll, inv, n):
    mats = np.concatenate([np.stack(family_members(n)), tie_batch(n) if n == 64 else shared_wave_batch()[0]])
    eye = np.broadcast_to(np.eye(n, dtype=np.float32), mats.shape).copy()
    assert inv.resolved_solve(n, n)[1:] == ((1, 64, 0) if n == 20 else (1, 0, 40))
    x, st = _check(dll, inv, mats, eye, tag="identity")
    want, want_st = inv.inv(torch.from_numpy(mats).cuda())
    torch.cuda.synchronize()
    want, want_st = want.cpu().numpy(), want_st.cpu().numpy()
    assert np.array_equal(st, want_st) and (st == 0).sum() >= 4
    for m in range(len(mats)):
        if st[m] == 0:
            assert np.array_equal(x[m], want[m]), (n, m)


def test_in_place_and_shapes(dll, inv):
    for n, k in ((20, 5), (100, 7), (8, 130)):
        mats = np.stack(family_members(n))
        b = _rhs_batch(mats, k)
        x, st = _check(dll, inv, mats, b, tag="out of place")
        ta, tb = torch.from_numpy(mats).cuda(), torch.from_numpy(b).cuda()
        x2, st2 = inv.solve(ta, tb, out=tb)
        torch.cuda.synchronize()
        assert x2.data_ptr() == tb.data_ptr() and np.array_equal(tb.cpu().numpy(), x), (n, k)
        assert np.array_equal(st2.cpu().numpy(), st)
        other = torch.full(b.shape, -7.5, device="cuda")
        status = torch.full((len(mats),), 9, dtype=torch.int32, device="cuda")
        x3, st3 = inv.solve(ta, torch.from_numpy(b).cuda(), out=other, status=status)
        torch.cuda.synchronize()
        assert x3.data_ptr() == other.data_ptr() and st3.data_ptr() == status.data_ptr()
        assert np.array_equal(other.cpu().numpy(), x) and not status.any().item()
    # one vector per member: (B, N) in, (B, N) out
    mats = np.stack(family_members(33))
    b = _rhs_batch(mats, 1)
    x, st = _check(dll, inv, mats, b, tag="vector")
    xv, stv = _solve(inv, mats, b[:, :, 0])
    assert xv.shape == (4, 33) and np.array_equal(xv, x[:, :, 0]) and np.array_equal(stv, st)
    # a 2-D a with a 1-D b, and with an (N, K) b
    xv, stv = _solve(inv, mats[2], b[2, :, 0])
    assert xv.shape == (33,) and stv.shape == (1,) and np.array_equal(xv, x[2, :, 0])
    xm, stm = _solve(inv, mats[2], b[2])
    assert xm.shape == (33, 1) and np.array_equal(xm, x[2])
    # a non-contiguous b is read through a contiguous copy
    wide = torch.from_numpy(_rhs_batch(mats, 4)).cuda()
    xs, _ = inv.solve(torch.from_numpy(mats).cuda(), wide[:, :, 1:3])
    torch.cuda.synchronize()
    want, _ = mirror_solve_batch(dll, mats, wide[:, :, 1:3].cpu().numpy())
    assert np.array_equal(xs.cpu().numpy(), want)


def test_large_batches(dll, inv):
    n, batch, k = 5, 70_000, 3     # every group of 8 lanes is full; more groups than one grid dimension of 65 535 holds
    mats = big_batch(n, batch)
    b = np.random.default_rng(77).uniform(-1, 1, (batch, n, k)).astype(np.float32)
    want_x, want_st = mirror_solve_batch(dll, mats, b)
    x, st = _solve(inv, mats, b)
    assert not want_st.any() and not st.any()
    assert np.array_equal(x, want_x)                             # every member, none sampled
    n, batch, distinct = 70, 66_000, 64                          # more workgroups than 65 535
    base = np.stack([dist for s in range(distinct // 4) for dist in family_members(n)][:distinct])
    base = base * np.linspace(0.5, 1.5, distinct, dtype=np.float32)[:, None, None]   # 64 distinct matrices
    base_b = _rhs_batch(base, 1)
    want_x, want_st = mirror_solve_batch(dll, base, base_b)
    assert not want_st.any() and len({m.tobytes() for m in base}) == distinct
    idx = torch.arange(batch, device="cuda") % distinct
    ta = torch.from_numpy(base).cuda()[idx]                      # tiled on the device
    tb = torch.from_numpy(base_b).cuda()[idx]
    x, st = inv.solve(ta, tb)
    torch.cuda.synchronize()
    assert not st.any().item()
    assert torch.equal(x, torch.from_numpy(want_x).cuda()[idx])  # each value against the mirror of its matrix


def test_argument_errors(inv):
    a = torch.eye(8, device="cuda").repeat(3, 1, 1)
    b = torch.ones(3, 8, 2, device="cuda")
    with pytest.raises(ValueError):
        inv.solve(a, b.double())                                 # dtype mismatch
    with pytest.raises(ValueError):
        inv.solve(a, b.cpu())                                    # wrong device
    with pytest.raises(ValueError):
        inv.solve(a.cpu(), b.cpu())
    with pytest.raises(ValueError):
        inv.solve(a.half(), b.half())
    with pytest.raises(ValueError):
        inv.solve(torch.eye(128, device="cuda"), torch.ones(128, 1, device="cuda"))   # no spare column
    with pytest.raises(ValueError):
        inv.solve(torch.eye(200, device="cuda"), torch.ones(200, 1, device="cuda"))
    with pytest.raises(ValueError):
        inv.solve(a, torch.ones(3, 7, 2, device="cuda"))         # b rows != N
    with pytest.raises(ValueError):
        inv.solve(a, torch.ones(2, 8, 2, device="cuda"))         # another batch
    with pytest.raises(ValueError):
        inv.solve(a, torch.ones(3, 8, 0, device="cuda"))         # no column
    with pytest.raises(ValueError):
        inv.solve(a, b, out=torch.empty(3, 8, 3, device="cuda"))  # out of another shape
    with pytest.raises(ValueError):
        inv.solve(a, b, out=torch.empty(3, 2, 8, device="cuda").transpose(1, 2))   # not contiguous
    with pytest.raises(ValueError):
        inv.resolved_solve(128, 1)
    with pytest.raises(ValueError):
        inv.resolved_solve(8, 0)
    x, st = inv.solve(a, b)                                      # and the call these refuse to be: X = B for A = I
    torch.cuda.synchronize()
    assert torch.equal(x, b) and st.tolist() == [0, 0, 0]
