"""GPU tests of the determinant beside the inverse above order 128 (``Inverter.inv_det_any``,
``mi32_inv_det_any_device*``; run with ``-m gpu`` on an MI355X): the sweep and the blocked paths, fp32 and fp64, with
partial pivoting and without, one block and several, batches, shared panels with the look-ahead, and a split batch.

There is no tolerance anywhere in this file.  Every case asserts three things: the inverse and status bytes equal
``inv``'s on the same ``Inverter``; the mantissa bit patterns and the exponents equal the pair the recurrence
(det_cases.frexp_det) gives on the pivots of the mirrors of tests/det_mirror_large.c -- (a) the step-by-step order, or
(b) the fp64 blocked order for the pivoted fp64 blocked path --, which tests/test_det_large_mirror.py holds to the
oracle; and the status equals the oracle's.  The shapes are the smallest that reach each code path.
"""
import math

import numpy as np
import pytest

import tall_batch_cases as tall
from degenerate_cases import zero_column, zero_row
from det_cases import dominant_member, family_members, permutation_matrix, same_doubles
from det_large_cases import (build_mirror_large, expected_pair, mirror_blocked64, mirror_steps, signed_power_diagonal)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_matrix_inversion_amd as g  # noqa: E402


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return build_mirror_large(tmp_path_factory.mktemp("det_mirror_large"))


def _np(t):
    return None if t is None else t.cpu().numpy()


def _run(inverter, mats, **kw):
    """inv and inv_det_any on the same Inverter; asserts the first thing (inverse and status bytes equal inv's) and
    returns (inverse, status, mant, exp) as numpy arrays."""
    t = torch.from_numpy(np.ascontiguousarray(mats)).cuda()
    x0, st0 = inverter.inv(t)
    x, st, mant, exp = inverter.inv_det_any(t, **kw)
    torch.cuda.synchronize()
    assert mant.dtype == torch.float64 and exp.dtype == torch.int32 and st.dtype == torch.int32
    x0, st0, x, st = _np(x0), _np(st0), _np(x), _np(st)
    assert np.array_equal(st, st0)
    if x is not None:
        assert x.tobytes() == x0.tobytes(), "inv_det_any's inverse is not inv's"
    return x, st, _np(mant), _np(exp)


def _oracle_status(oracle, a, pivoting, bw64=0):
    n = a.shape[0]
    if not pivoting:
        return oracle.matrix_inversion_no_pivots(a, n, return_info=True)[1]["status"]
    if a.dtype == np.float32:
        return oracle.matrix_inv_32_inplace(a, n, return_info=True)[1]["status"]
    if bw64:
        return oracle.matrix_inv_64_blocked(a, n, bw64, return_info=True)[1]["status"]
    return oracle.matrix_inv_64(a, n, return_info=True)[1]["status"]


def _check(oracle, dll, inverter, mats, pivoting=True, bw64=0, tag=None):
    """One call on the batch `mats` (B, N, N); bw64 > 0: mirror (b) with that width, else mirror (a)."""
    mats = np.ascontiguousarray(mats)
    x, st, mant, exp = _run(inverter, mats)
    want_m, want_e = [], []
    for b, a in enumerate(mats):
        mx, mst, piv, swp = mirror_blocked64(dll, a, bw64) if bw64 else mirror_steps(dll, a, pivoting)
        m, e = expected_pair(a, piv, swp, pivoting)
        want_m.append(m)
        want_e.append(e)
        assert st[b] == mst == _oracle_status(oracle, a, pivoting, bw64), (tag, b, st[b], mst)
        if mst == 0:
            assert np.array_equal(x[b], mx), (tag, b)
    print(tag, "mant", mant, "exp", exp)
    assert same_doubles(mant, np.array(want_m)), (tag, mant, want_m)
    assert np.array_equal(exp, np.array(want_e, np.int32)), (tag, exp, want_e)
    return st, mant, exp


# ---- fp32, pivoting, AUTO: the blocked path -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [129, 200, 256, 257, 300])
def test_fp32_blocked_auto(oracle, dll, n):
    """129, 200, 256: one outer block (the whole matrix is the panel); 257 and 300: two.  A batch of the four families."""
    inv = g.Inverter()
    try:
        assert inv.resolved_algo(n, 4) == g.ALGO_BLOCKED
        route, _ = inv.resolved_route(n, 4)
        assert route["nblocks"] == (1 if n <= 256 else 2)
        st, mant, _ = _check(oracle, dll, inv, np.stack(family_members(n)), tag=f"fp32 auto {n}")
        assert not st.any() and (np.abs(mant) >= 0.5).all() and (np.abs(mant) < 1.0).all()
    finally:
        inv.close()


@pytest.mark.parametrize("n,w,blocks", [(300, 8, 3), (300, 32, 3), (640, 8, 5), (640, 32, 5)])
def test_fp32_blocked_forced_blocks(oracle, dll, n, w, blocks):
    """Three and five outer blocks at block_width = 128 (the shapes of subnormal_cases.BLOCKED32_BW128): mf[blk & 1] is
    reused by the block after next."""
    inv = g.Inverter(panel_width=w, block_width=128)
    try:
        route, _ = inv.resolved_route(n, 1)
        assert route["nblocks"] == blocks and route["block_width"] == 128
        st, _, _ = _check(oracle, dll, inv, np.stack(family_members(n)[:2]), tag=f"fp32 bw128 {n} w{w}")
        assert not st.any()
    finally:
        inv.close()


# ---- fp32, other routes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [129, 131, 300])
def test_fp32_sweep(oracle, dll, n):
    inv = g.Inverter(algo="sweep")
    try:
        assert inv.resolved_algo(n, 4) == g.ALGO_SWEEP
        st, _, _ = _check(oracle, dll, inv, np.stack(family_members(n)), tag=f"fp32 sweep {n}")
        assert not st.any()
    finally:
        inv.close()


@pytest.mark.parametrize("n,algo", [(200, g.ALGO_SWEEP), (513, g.ALGO_BLOCKED), (640, g.ALGO_BLOCKED)])
def test_fp32_no_pivot(oracle, dll, n, algo):
    inv = g.Inverter(pivoting=False)
    try:
        assert inv.resolved_algo(n, 1) == algo
        st, mant, _ = _check(oracle, dll, inv, dominant_member(n, np.float32)[None], pivoting=False,
                             tag=f"fp32 nopivot {n}")
        assert not st.any() and (mant > 0).all()  # strictly diagonally dominant with a positive diagonal
    finally:
        inv.close()


# ---- fp64 ---------------------------------------------------------------------------------------------------------------
def _fp64_members(n):
    return np.stack(family_members(n, np.float64)) * 1.000000001  # entries that are no float32 values


@pytest.mark.parametrize("n", [129, 255])
def test_fp64_sweep(oracle, dll, n):
    inv = g.Inverter()
    try:
        assert inv.resolved_blocking_f64(n) == 0
        st, _, _ = _check(oracle, dll, inv, _fp64_members(n), tag=f"fp64 sweep {n}")
        assert not st.any()
    finally:
        inv.close()


@pytest.mark.parametrize("n", [256, 300, 700])
def test_fp64_blocked_pivoting(oracle, dll, n):
    """Against mirror (b), with the width resolved_blocking_f64 reports."""
    inv = g.Inverter()
    try:
        bw = inv.resolved_blocking_f64(n)
        assert bw > 0
        st, _, _ = _check(oracle, dll, inv, _fp64_members(n)[:2], bw64=bw, tag=f"fp64 blocked {n} bw{bw}")
        assert not st.any()
    finally:
        inv.close()


def test_fp64_no_pivot_sweep(oracle, dll):
    inv = g.Inverter(pivoting=False)
    try:
        assert inv.resolved_blocking_f64(300) == 0
        st, _, _ = _check(oracle, dll, inv, dominant_member(300, np.float64)[None], pivoting=False, tag="fp64 nopivot 300")
        assert not st.any()
    finally:
        inv.close()


@pytest.mark.parametrize("n", [512, 700])
@pytest.mark.parametrize("bw", [64, 128])
def test_fp64_no_pivot_blocked(oracle, dll, n, bw):
    inv = g.Inverter(pivoting=False, block_width=bw)
    try:
        assert inv.resolved_blocking_f64(n) == bw
        st, mant, _ = _check(oracle, dll, inv, dominant_member(n, np.float64)[None], pivoting=False,
                             tag=f"fp64 nopivot {n} bw{bw}")
        assert not st.any() and (mant > 0).all()
    finally:
        inv.close()


# ---- special values -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["auto", "sweep"])
def test_permutation_matrices(oracle, dll, algo):
    inv = g.Inverter(algo=algo)
    try:
        for n in (129, 300):
            for dtype in (np.float32, np.float64):
                mats = np.stack([permutation_matrix(n, False, dtype), permutation_matrix(n, True, dtype)])
                bw = inv.resolved_blocking_f64(n) if dtype == np.float64 else 0
                st, mant, exp = _check(oracle, dll, inv, mats, bw64=bw, tag=f"perm {algo} {n}")
                assert not st.any() and mant.tolist() == [0.5, -0.5] and exp.tolist() == [1, 1]
    finally:
        inv.close()


def test_extreme_exponents(oracle, dll):
    """diag(2^100) and diag(2^-120) at N = 200 in fp32: exponents +-20 000 and more; diag(2^+-1000) in fp64."""
    for algo in ("auto", "sweep"):
        inv = g.Inverter(algo=algo)
        try:
            n = 200
            for k, dtype in ((100, np.float32), (-120, np.float32), (1000, np.float64), (-1000, np.float64)):
                a = np.diag(np.full(n, 2.0 ** k)).astype(dtype)
                st, mant, exp = _check(oracle, dll, inv, a[None], tag=f"diag {algo} 2^{k}")
                assert not st.any() and mant.tolist() == [0.5] and exp.tolist() == [k * n + 1]
        finally:
            inv.close()


# ---- flagged members ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["auto", "sweep"])
def test_flagged_members(oracle, dll, algo):
    n = 200
    good = family_members(n)[0]
    nan_in = good.copy()
    nan_in[n - 3, 7] = np.nan
    inf_in = good.copy()
    inf_in[5, n - 2] = np.inf
    mats = np.stack([good, zero_column(n, 77, 11), zero_row(n, 50, 12), nan_in, inf_in, family_members(n)[1]])
    inv = g.Inverter(algo=algo)
    try:
        st, mant, exp = _check(oracle, dll, inv, mats, tag=f"flagged {algo}")
    finally:
        inv.close()
    assert st.tolist() == [0, 2, 2, 2, 2, 0]
    assert mant[1] == 0.0 and not np.signbit(mant[1]) and exp[1] == 0        # a zero column: (+0.0, 0)
    assert mant[2] == 0.0 and not np.signbit(mant[2]) and exp[2] == 0        # singular at the last step
    assert math.isnan(mant[3]) and exp[3] == 0 and math.isnan(mant[4]) and exp[4] == 0
    # with pivoting off a zero diagonal entry: (NaN, 0)
    hit = dominant_member(n, np.float32)
    hit[100, :] = 0.0
    hit[:, 100] = 0.0  # stays exactly zero: the entry is untouched by every earlier step
    inv = g.Inverter(algo=algo, pivoting=False)
    try:
        st, mant, exp = _check(oracle, dll, inv, np.stack([dominant_member(n, np.float32), hit, dominant_member(n, np.float32)]),
                               pivoting=False, tag=f"flagged nopivot {algo}")
    finally:
        inv.close()
    assert st.tolist() == [0, 2, 0] and math.isnan(mant[1]) and exp[1] == 0 and mant[0] > 0 and mant[2] == mant[0]


# ---- above 4096 padded rows: shared panels, look-ahead, second stream -----------------------------------------------------
@pytest.fixture(scope="module")
def tall_gate(dll):
    """gate_matrix(4200, 40 000), the single matrix of the shared-panel tests, and mirror (a) on it: the one long CPU
    step of this file."""
    a = tall.cached_base("gate", tall.N_TALL, tall.SEED_GATE)
    return a, mirror_steps(dll, a)


def test_shared_panels_and_lookahead(oracle, dll, tall_gate):
    a, (mx, mst, piv, swp) = tall_gate
    n = a.shape[0]
    inv = g.Inverter()
    try:
        route, groups = inv.resolved_route(n, 1)
        assert route["shared_panels"] and route["lookahead"] and groups[0] == 2
        x, st, mant, exp = _run(inv, a[None])
    finally:
        inv.close()
    m, e = expected_pair(a, piv, swp)
    print("N 4200 pair", mant, exp, "want", m, e)
    assert st[0] == mst == 0
    assert np.array_equal(x[0], mx)
    assert np.array_equal(x[0], tall.oracle_inverse(oracle, ("gate", n, tall.SEED_GATE)).reshape(n, n))
    assert same_doubles(mant, np.array([m])) and exp[0] == e


@pytest.mark.parametrize("n", [300, tall.N_TALL, tall.N_WIDE])
def test_signed_power_diagonal_closed_form(dll, n):
    """P D, D a diagonal of signed powers of two: the pair is known in closed form (checked against the mirror at
    N = 300 here and in tests/test_det_large_mirror.py).  4200 and 8200: two and three workgroups per shared panel."""
    a, mant_want, exp_want = signed_power_diagonal(n, n)
    inv = g.Inverter()
    try:
        x, st, mant, exp = _run(inv, a[None])
        x2, st2, mant2, exp2 = _run(inv, a[None], want_inverse=False)
    finally:
        inv.close()
    assert st[0] == 0 and st2[0] == 0 and x2 is None
    assert same_doubles(mant, np.array([mant_want])) and exp[0] == exp_want
    assert same_doubles(mant2, np.array([mant_want])) and exp2[0] == exp_want
    if n == 300:
        mx, mst, piv, swp = mirror_steps(dll, a)
        assert expected_pair(a, piv, swp) == (mant_want, exp_want) and np.array_equal(x[0], mx)
    # the inverse of P D is D^-1 P^T, exactly
    nz = np.nonzero(a)
    want = np.zeros_like(a)
    want[nz[1], nz[0]] = np.float32(1.0) / a[nz]
    assert np.array_equal(x[0], want)


def test_split_batch_with_a_bad_member(oracle, dll):
    """The smallest shape of tall_batch_cases for which resolved_route reports two parts (4200 x 5: three members on
    the main stream, two on the split stream), with a bad member in the second part.  The members are exact: P D of
    signed powers of two, and a zero column in member 3."""
    n, batch = tall.N_TALL, 5
    inv = g.Inverter()
    try:
        route, _ = inv.resolved_route(n, batch)
        assert route["parts"] == 2 and route["part_batch"] == [3, 2]
        made = [signed_power_diagonal(n, 100 + b) for b in range(batch)]
        mats = np.stack([m[0] for m in made])
        mats[3][:, np.nonzero(mats[3][17])[0][0]] = 0.0  # row 17's entry was its column's only one
        x, st, mant, exp = _run(inv, mats)
    finally:
        inv.close()
    assert st.tolist() == [0, 0, 0, 2, 0]
    for b in (0, 1, 2, 4):
        assert same_doubles(mant[b:b + 1], np.array([made[b][1]])) and exp[b] == made[b][2], b
    assert mant[3] == 0.0 and not np.signbit(mant[3]) and exp[3] == 0


# ---- delegation and forms -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 128])
def test_small_orders_are_inv_det(n):
    inv = g.Inverter()
    try:
        for mats in (np.stack(family_members(n)), _fp64_members(n)):
            t = torch.from_numpy(mats).cuda()
            x0, st0, m0, e0 = inv.inv_det(t)
            x, st, m, e = inv.inv_det_any(t)
            torch.cuda.synchronize()
            assert _np(x).tobytes() == _np(x0).tobytes() and np.array_equal(_np(st), _np(st0))
            assert _np(m).tobytes() == _np(m0).tobytes() and np.array_equal(_np(e), _np(e0))
    finally:
        inv.close()


@pytest.mark.parametrize("algo,pivoting,dtype,n", [("auto", True, np.float32, 300), ("sweep", True, np.float32, 200),
                                                   ("auto", False, np.float32, 513), ("auto", True, np.float64, 300),
                                                   ("auto", True, np.float64, 200), ("auto", False, np.float64, 512)])
def test_determinant_only(algo, pivoting, dtype, n):
    """want_inverse=False: the same status and pair, None for the inverse."""
    mats = np.stack(family_members(n, dtype)[:2]) if pivoting else dominant_member(n, dtype)[None]
    inv = g.Inverter(algo=algo, pivoting=pivoting)
    try:
        x, st, mant, exp = _run(inv, mats)
        x2, st2, mant2, exp2 = _run(inv, mats, want_inverse=False)
    finally:
        inv.close()
    assert x2 is None and np.array_equal(st, st2) and not st.any()
    assert mant.tobytes() == mant2.tobytes() and np.array_equal(exp, exp2)


# ---- sequences ------------------------------------------------------------------------------------------------------------
def test_back_to_back_on_one_context(oracle, dll):
    """inv_det_any at N = 300, then at N = 129, then inv at N = 300, on one context and one stream with no
    synchronisation in between; all three results are checked afterwards."""
    a300 = np.stack(family_members(300))
    a129 = np.stack(family_members(129))
    inv = g.Inverter()
    try:
        t300, t129 = torch.from_numpy(a300).cuda(), torch.from_numpy(a129).cuda()
        torch.cuda.synchronize()
        r1 = inv.inv_det_any(t300)
        r2 = inv.inv_det_any(t129)
        r3 = inv.inv(t300)
        torch.cuda.synchronize()
    finally:
        inv.close()
    for mats, (x, st, mant, exp) in ((a300, r1), (a129, r2)):
        x, st, mant, exp = _np(x), _np(st), _np(mant), _np(exp)
        for b, a in enumerate(mats):
            mx, mst, piv, swp = mirror_steps(dll, a)
            m, e = expected_pair(a, piv, swp)
            assert st[b] == mst == 0 and np.array_equal(x[b], mx)
            assert same_doubles(mant[b:b + 1], np.array([m])) and exp[b] == e
    assert _np(r3[0]).tobytes() == _np(r1[0]).tobytes() and not _np(r3[1]).any()
