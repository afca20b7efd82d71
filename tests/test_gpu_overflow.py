"""GPU tests of every inversion route on inputs whose INVERSE overflows while the status stays 0 (run with ``-m gpu`` on
an MI355X).  The inputs, the route table and the reference of every route are those of tests/overflow_cases.py;
tests/test_overflow_cases.py proves on the CPU that every entry is status 0 with a mostly finite result holding
infinities and NaN, and that the two rules for a zero multiplier part on the block-diagonal entries.

There is no tolerance anywhere in this file.  A status is compared with the reference's; a result with
``overflow_cases.same_with_nonfinite``: the same positions of non-finite entries, infinities with their sign, every NaN
one value, the finite entries byte for byte (-0.0 stored as +0.0).  Every test body asserts that what it compared held
infinities.  Which reference a route is held to is decided in the table, not read off the code under test:

  * the sweep and the one-launch routes: the step-by-step oracle, which skips an exact-zero multiplier;
  * the blocked fp32 route and the fp64 no-pivot blocked one: the same oracle multiplying a zero multiplier through;
  * the fp64 blocked route: its composite-order mirror ``matrix_inv_64_blocked`` at the resolved block width.
"""
import numpy as np
import pytest

import overflow_cases as C
import subnormal_cases as S
from batch_helpers import strided
from det_cases import build_mirror, expected, same_doubles
from det_large_cases import build_mirror_large, expected_pair, mirror_blocked64, mirror_steps
from resident_cases import run
from solve_cases import build_solve_mirror, mirror_solve, mirror_solve_batch, rhs
from vbatch_cases import pack, unpack

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_matrix_inversion_amd as g  # noqa: E402

F32, F64 = np.float32, np.float64
DTYPES = pytest.mark.parametrize("dtype", [F32, F64], ids=["fp32", "fp64"])
PIVOTING = pytest.mark.parametrize("pivoting", [True, False], ids=["pivot", "nopivot"])
OK = 0


def ident(c):
    n = "+".join(str(v) for v in c.n) if c.kind == "block_diag" else str(c.n)
    return f"{c.kind}-{'fp32' if c.dtype == F32 else 'fp64'}-{n}" + ("" if c.first else "-second") + \
        ("" if c.pivoting else "-nopivot")


def cases_of(*routes):
    return [pytest.param(c, id=ident(c)) for r in routes for c in C.ROUTES[r][1]]


def assert_same(got, want, tag, infinities=True):
    """``got`` is ``want`` under same_with_nonfinite -- and, unless the member is an ordinary one, what was compared
    held infinities."""
    got = np.ascontiguousarray(got)
    assert C.same_with_nonfinite(got, want), (tag, C.difference(got, want))
    if infinities:
        assert np.isinf(got).sum() >= 4, (tag, C.counts(got))
    else:
        assert np.isfinite(got).all(), tag


def check_case(oracle, inv, c, ref, tag, bw=None):
    want, st_want = C.reference(oracle, c, ref, bw)
    assert st_want == OK == g.MI32_OK
    got, st = run(inv, C.matrix(c))
    assert st.tolist() == [OK], (tag, c, st)
    assert_same(got, want, (tag, c))
    return got


def _inverter_fixture(**kw):
    @pytest.fixture(scope="module")
    def fx():
        inv = g.Inverter(**kw)
        try:
            yield inv
        finally:
            inv.close()
    return fx


inv_sweep = _inverter_fixture(algo="sweep")
inv_blocked = _inverter_fixture(algo="blocked")
inv_auto_nopivot = _inverter_fixture(algo="auto", pivoting=False)
inv_default = _inverter_fixture()


@pytest.fixture(scope="module")
def one_launch():
    """{pivoting: handle}: ``algo="workgroup"`` takes the register-resident kernels up to 64 rows and the
    workgroup-resident ones above."""
    invs = {p: g.Inverter(algo="workgroup", pivoting=p) for p in (True, False)}
    yield invs
    for inv in invs.values():
        inv.close()


@pytest.fixture(scope="module")
def plain_or_nopivot():
    """{pivoting: handle} on the default algorithm."""
    invs = {p: g.Inverter(pivoting=p) for p in (True, False)}
    yield invs
    for inv in invs.values():
        inv.close()


@pytest.fixture(scope="module")
def det_dll(tmp_path_factory):
    return build_mirror(tmp_path_factory.mktemp("det_mirror"))


@pytest.fixture(scope="module")
def det_large_dll(tmp_path_factory):
    return build_mirror_large(tmp_path_factory.mktemp("det_mirror_large"))


@pytest.fixture(scope="module")
def solve_dll(tmp_path_factory):
    return build_solve_mirror(tmp_path_factory.mktemp("solve_mirror"))


# ---- sweep: the reference's rule ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cases_of("sweep32", "sweep64", "sweep_nopivot"))
def test_sweep(oracle, inv_sweep, inv_auto_nopivot, c):
    """No-pivot at order 100: below 512 rows a single matrix takes the sweep on ``algo="auto"``."""
    inv = inv_sweep if c.pivoting else inv_auto_nopivot
    n = C.order(c)
    assert inv.resolved_algo(n, 1) == g.ALGO_SWEEP and inv.resolved_blocking_f64(n) == 0
    check_case(oracle, inv, c, "skip", "sweep")


# ---- blocked fp32: a zero multiplier is multiplied through -------------------------------------------------------------
@pytest.mark.parametrize("c", cases_of("blocked32"))
def test_blocked_fp32_default_plan(oracle, inv_blocked, c):
    """16: one panel behind 112 padded rows; 130 and 300: two outer blocks of the default plan."""
    assert inv_blocked.resolved_algo(c.n, 1) == g.ALGO_BLOCKED
    check_case(oracle, inv_blocked, c, "through", "blocked")


@pytest.mark.parametrize("n,w", C.BLOCKED32_BW128)
def test_blocked_fp32_three_and_five_outer_blocks(oracle, n, w):
    """block_width = 128: outside-block strips and rank-bw updates on the matrix cores with infinities as the B operand,
    at a narrow and at a wide sub-panel."""
    inv = g.Inverter(algo="blocked", panel_width=w, block_width=128)
    try:
        assert inv.resolved_algo(n, 1) == g.ALGO_BLOCKED and inv.resolved_blocking(n, 1) == (w, 128)
        widths = inv.resolved_panel_widths(n, 1)
        assert len(widths) == -(-n // 128) == {300: 3, 640: 5}[n] and widths[0] == w
        ran = [check_case(oracle, inv, c, "through", ("blocked bw 128", w)) for c in C.ROUTES["blocked32_bw128"][1]
               if c.n == n]
        assert len(ran) == 1
    finally:
        inv.close()


@pytest.mark.parametrize("c", cases_of("blocked32_block_diag"))
def test_blocked_fp32_block_diagonal(oracle, inv_blocked, c):
    """Every multiplier between the blocks is an exact zero and the pivot rows of the overflowing block hold infinities:
    fma(-0, +-inf, x) = NaN on this route where the sweep keeps x.  The multiply-through oracle is the reference, and
    the skip oracle's result is NOT what comes out (tests/test_overflow_cases.py: they differ in >= n entries)."""
    n = C.order(c)
    assert inv_blocked.resolved_algo(n, 1) == g.ALGO_BLOCKED
    got = check_case(oracle, inv_blocked, c, "through", "blocked block_diag")
    assert not C.same_with_nonfinite(got, C.reference(oracle, c, "skip")[0])


def test_blocked_fp32_batch(oracle, inv_blocked):
    """rows_down, both block_diag orders and an ordinary member in one call: the ordinary member stays byte-identical to
    its solo result."""
    n = C.BLOCKED32_BATCH_ORDER
    cs = [C.case("rows_down", F32, n), C.case("block_diag", F32, (150, 150)),
          C.case("block_diag", F32, (150, 150), first=False), C.case("plain", F32, n)]
    assert all(c in C.ROUTES["blocked32"][1] + C.ROUTES["blocked32_block_diag"][1] for c in cs[:3])
    assert inv_blocked.resolved_algo(n, len(cs)) == g.ALGO_BLOCKED
    mats = np.stack([C.matrix(c) for c in cs])
    got, st = run(inv_blocked, mats)
    assert st.tolist() == [OK] * 4
    for b, c in enumerate(cs[:3]):
        assert_same(got[b], C.reference(oracle, c, "through")[0], ("blocked batch", b, c))
    solo, st1 = run(inv_blocked, mats[3])
    assert st1.tolist() == [OK] and np.isfinite(solo).all() and got[3].tobytes() == solo.tobytes()
    want, info = oracle.matrix_inv_32_inplace(mats[3], n, return_info=True)
    assert info["status"] == OK
    assert_same(got[3], want.reshape(n, n), "blocked batch, ordinary member", infinities=False)


@pytest.mark.parametrize("c", cases_of("blocked32_nopivot", "nopivot64_blocked"))
def test_no_pivot_blocked(oracle, inv_auto_nopivot, c):
    """From 512 rows on: the blocked fp32 path in its no-pivot shape and mi32_nopivot64.hip (520: padded to 576, 640:
    not padded), both against the no-pivot step oracle multiplying a zero multiplier through."""
    inv, n = inv_auto_nopivot, C.order(c)
    if c.dtype == F32:
        assert inv.resolved_algo(n, 1) == g.ALGO_BLOCKED
    else:
        assert inv.resolved_blocking_f64(n) > 0
    got = check_case(oracle, inv, c, "through", "no pivot blocked")
    if c.kind == "block_diag":
        assert not C.same_with_nonfinite(got, C.reference(oracle, c, "skip")[0])


# ---- fp64 blocked: the composite-order mirror --------------------------------------------------------------------------
@pytest.mark.parametrize("bw_req", [0, 64])
@pytest.mark.parametrize("c", cases_of("blocked64"))
def test_blocked_fp64(oracle, c, bw_req):
    """n = 300: padded to 320 (width 64) and to 384 (the default width); n = 256: no padding, the control."""
    inv = g.Inverter(algo="auto", block_width=bw_req)
    try:
        bw = inv.resolved_blocking_f64(C.order(c))
        assert bw in C.F64_BLOCKED_WIDTHS and (bw_req == 0 or bw == bw_req)
        if bw not in C.widths_of("blocked64", c):
            assert c.n == 256 and bw == 64 and 128 in C.widths_of("blocked64", c)
            bw = 0          # the control runs at the default width only
        if bw:
            check_case(oracle, inv, c, "mirror64", ("blocked fp64", bw), bw=bw)
    finally:
        inv.close()


@pytest.mark.parametrize("bw_req", [0, 64])
def test_blocked_fp64_follows_the_mirrors_overflow_boundary(oracle, bw_req):
    """n = 300, s = 1028: the step oracle inverts it (status 0), the composite order flags it: the status is the
    mirror's.  The output is not compared."""
    c = C.BLOCKED64_STATUS2
    inv = g.Inverter(algo="auto", block_width=bw_req)
    try:
        bw = inv.resolved_blocking_f64(c.n)
        assert C.reference(oracle, c, "skip")[1] == OK and C.reference(oracle, c, "mirror64", bw)[1] == C.SINGULAR
        _, st = run(inv, C.matrix(c))
        assert st.tolist() == [C.SINGULAR] == [g.MI32_SINGULAR]
    finally:
        inv.close()


# ---- resident and workgroup --------------------------------------------------------------------------------------------
def _check_mixed_batch(oracle, inv, mats, cs, tag):
    got, st = run(inv, mats)
    assert got.dtype == mats.dtype and st.tolist() == [OK] * len(cs), (tag, st)
    kinds = set()
    for b, c in enumerate(cs):
        want, st_want = C.reference(oracle, c, "skip")
        assert st_want == OK
        assert_same(got[b], want, (tag, b, c), infinities=c.kind != "plain")
        kinds.add(c.kind)
    assert kinds == {"rows_down", "block_diag", "plain"}, tag
    return got


@DTYPES
@PIVOTING
@pytest.mark.parametrize("n", S.RESIDENT_ORDERS)
def test_resident_mixed_batch(oracle, one_launch, n, pivoting, dtype):
    inv = one_launch[pivoting]
    assert inv.resolved_algo(n, S.RESIDENT_BATCH) == g.ALGO_RESIDENT
    mats, cs = C.mixed_batch(n, S.RESIDENT_BATCH, dtype, pivoting)
    _check_mixed_batch(oracle, inv, mats, cs, ("resident", n, pivoting))


@DTYPES
@PIVOTING
@pytest.mark.parametrize("n", S.WORKGROUP_ORDERS)
def test_workgroup_mixed_batch(oracle, one_launch, n, pivoting, dtype):
    inv = one_launch[pivoting]
    assert inv.resolved_algo(n, S.WORKGROUP_BATCH) == g.ALGO_WORKGROUP
    mats, cs = C.mixed_batch(n, S.WORKGROUP_BATCH, dtype, pivoting)
    _check_mixed_batch(oracle, inv, mats, cs, ("workgroup", n, pivoting))


# ---- mixed orders in one call ------------------------------------------------------------------------------------------
def _ragged_members(oracle, dtype, pivoting):
    """RAGGED_ORDERS three times over, the three kinds in turn (order 3 travels as an ordinary member)."""
    orders = S.RAGGED_ORDERS * S.RAGGED_COPIES
    cs = [C.one_launch_cases(n, dtype, pivoting)[b % 3] for b, n in enumerate(orders)]
    want = [C.reference(oracle, c, "skip") for c in cs]
    assert [s for _, s in want] == [OK] * len(cs)
    assert {c.kind for c in cs if c.n != 3} == {"rows_down", "block_diag", "plain"}
    return [C.matrix(c) for c in cs], cs, [x for x, _ in want]


def _assert_ragged(got, cs, want, tag):
    for b, c in enumerate(cs):
        assert_same(got[b], want[b], (tag, b, c), infinities=c.kind != "plain")


@DTYPES
@PIVOTING
def test_ragged_call_packed(oracle, plain_or_nopivot, dtype, pivoting):
    inv = plain_or_nopivot[pivoting]
    mats, cs, want = _ragged_members(oracle, dtype, pivoting)
    orders, flat = pack(mats)
    plan = inv.plan_ragged(orders)
    try:
        x, st = inv.inv_ragged(plan, torch.from_numpy(flat).cuda())
        torch.cuda.synchronize()
    finally:
        plan.close()
    assert st.cpu().numpy().tolist() == [OK] * len(mats)
    _assert_ragged(unpack(x.cpu().numpy(), orders), cs, want, "ragged")


@DTYPES
@PIVOTING
def test_ragged_call_strided_between_nan_padding(oracle, plain_or_nopivot, dtype, pivoting):
    inv = plain_or_nopivot[pivoting]
    mats, cs, want = _ragged_members(oracle, dtype, pivoting)
    tdt, es = (torch.float32, 4) if dtype == F32 else (torch.float64, 8)
    sentinel = dtype(-12345.5)
    a_buf, a_off, lda, _ = strided(mats, 3, np.nan)            # NaN in the input padding: never read
    o_buf, o_off, ldo, o_pad = strided([np.zeros_like(m) for m in mats], 5, sentinel)
    o_buf[:] = sentinel
    ta, to = torch.from_numpy(a_buf).cuda(), torch.from_numpy(o_buf).cuda()
    plan = inv.plan_ragged([m.shape[0] for m in mats])
    try:
        st = inv.inv_pointers(plan, torch.from_numpy(a_off * es + ta.data_ptr()).cuda(),
                              torch.from_numpy(o_off * es + to.data_ptr()).cuda(), tdt,
                              lda=torch.from_numpy(lda).cuda(), ldout=torch.from_numpy(ldo).cuda())
        torch.cuda.synchronize()
    finally:
        plan.close()
    out = to.cpu().numpy()
    assert st.cpu().numpy().tolist() == [OK] * len(mats)
    assert (out[o_pad] == sentinel).all()
    got = [out[o_off[b]:o_off[b] + m.shape[0] * ldo[b]].reshape(m.shape[0], ldo[b])[:, :m.shape[0]]
           for b, m in enumerate(mats)]
    _assert_ragged(got, cs, want, "strided")


# ---- the determinant beside the inverse --------------------------------------------------------------------------------
def _assert_pair(mant, exp, want_m, want_e, tag):
    """Every pivot is finite, so the pair is: bit for bit the mirror's recurrence."""
    assert np.isfinite(want_m).all() and (np.abs(want_m) >= 0.5).all() and (np.abs(want_m) < 1.0).all(), tag
    assert same_doubles(mant, want_m) and np.array_equal(exp, want_e), (tag, mant, want_m, exp, want_e)


@DTYPES
@PIVOTING
@pytest.mark.parametrize("n", C.DET_ORDERS)
def test_inv_det(oracle, det_dll, one_launch, n, pivoting, dtype):
    """On ``algo="workgroup"``, so that the plain call runs the one-launch kernels that ``inv_det`` always runs (on
    ``algo="auto"`` a small fp32 batch of these orders takes the blocked route, whose block_diag result is another)."""
    inv = one_launch[pivoting]
    assert inv.resolved_algo(n, 3) in (g.ALGO_RESIDENT, g.ALGO_WORKGROUP)
    cs = C.one_launch_cases(n, dtype, pivoting)
    mats = np.stack([C.matrix(c) for c in cs])
    _, want_st, want_m, want_e = expected(det_dll, mats, pivoting)
    t = torch.from_numpy(mats).cuda()
    x, st, mant, exp = inv.inv_det(t)
    plain, plain_st = inv.inv(t)
    none, st2, mant2, exp2 = inv.inv_det(t, want_inverse=False)
    torch.cuda.synchronize()
    assert none is None and torch.equal(st, plain_st) and torch.equal(st, st2)
    assert st.cpu().numpy().tolist() == want_st.tolist() == [OK] * len(cs)
    _assert_pair(mant.cpu().numpy(), exp.cpu().numpy(), want_m, want_e, ("inv_det", n))
    _assert_pair(mant2.cpu().numpy(), exp2.cpu().numpy(), want_m, want_e, ("inv_det, no inverse", n))
    x, plain = x.cpu().numpy(), plain.cpu().numpy()
    for b, c in enumerate(cs):
        assert_same(x[b], plain[b], ("inv_det against inv", n, b), infinities=c.kind != "plain")
        assert_same(x[b], C.reference(oracle, c, "skip")[0], ("inv_det", n, b), infinities=c.kind != "plain")


def _det_any(oracle, det_large_dll, inv, c, ref, bw=None):
    a = C.matrix(c)
    if bw:
        _, mst, piv, swp = mirror_blocked64(det_large_dll, a, bw)
    else:
        _, mst, piv, swp = mirror_steps(det_large_dll, a, c.pivoting)
    want_m, want_e = expected_pair(a, piv, swp, c.pivoting)
    assert mst == OK and np.isfinite(piv).all()
    t = torch.from_numpy(a[None]).cuda()
    x, st, mant, exp = inv.inv_det_any(t)
    plain, plain_st = inv.inv(t)
    none, st2, mant2, exp2 = inv.inv_det_any(t, want_inverse=False)
    torch.cuda.synchronize()
    assert none is None and st.tolist() == plain_st.tolist() == st2.tolist() == [OK]
    for m, e in ((mant, exp), (mant2, exp2)):
        _assert_pair(m.cpu().numpy(), e.cpu().numpy(), np.array([want_m]), np.array([want_e], np.int32), ("inv_det_any", c))
    x = x.cpu().numpy()[0]
    assert_same(x, plain.cpu().numpy()[0], ("inv_det_any against inv", c))
    assert_same(x, C.reference(oracle, c, ref, bw)[0], ("inv_det_any", c))


@pytest.mark.parametrize("c", cases_of("det_large32", "det_large64"))
def test_inv_det_any_blocked(oracle, det_large_dll, inv_default, c):
    """Order 300: the blocked fp32 route (padding first: ``det_first``) and the fp64 blocked one (padding behind)."""
    if c.dtype == F32:
        assert inv_default.resolved_algo(c.n, 1) == g.ALGO_BLOCKED
        _det_any(oracle, det_large_dll, inv_default, c, "through")
    else:
        bw = inv_default.resolved_blocking_f64(c.n)
        assert bw == 128
        _det_any(oracle, det_large_dll, inv_default, c, "mirror64", bw)


@pytest.mark.parametrize("c", cases_of("det_large_nopivot"))
def test_inv_det_any_no_pivot_blocked(oracle, det_large_dll, inv_auto_nopivot, c):
    """Order 520 on both no-pivot blocked paths (fp64: the padding comes first, its steps are skipped by index)."""
    inv = inv_auto_nopivot
    assert (inv.resolved_algo(c.n, 1) == g.ALGO_BLOCKED) if c.dtype == F32 else (inv.resolved_blocking_f64(c.n) > 0)
    _det_any(oracle, det_large_dll, inv, c, "through")


# ---- A X = B -----------------------------------------------------------------------------------------------------------
def _solve_systems(dtype):
    cs = [C.case("rows_down", dtype, n) for n in C.SOLVE_ORDERS]
    assert all(c in C.ROUTES["one_launch"][1] for c in cs)
    return cs, [C.matrix(c) for c in cs], [rhs(c.n, C.SOLVE_K, 8100 + c.n, dtype) for c in cs]


def _assert_solve(x, want, tag):
    """X against the solve mirror, its non-finite pattern included.  Every entry of X takes a part of every overflowing
    column of the inverse, so X is wholly non-finite: infinities (with their sign) at order 8, and from order 33 on NaN
    where infinities of both signs meet.  Returns the number of infinities compared; the callers assert that the call
    as a whole held some."""
    assert C.same_with_nonfinite(x, want), (tag, C.difference(x, want))
    assert not np.isfinite(x).all(), (tag, C.counts(x))
    return int(np.isinf(x).sum())


@DTYPES
def test_solve(solve_dll, inv_default, dtype):
    infs = 0
    for c, a, b in zip(*_solve_systems(dtype)):
        want, want_st = mirror_solve_batch(solve_dll, a[None], b[None])
        x, st = inv_default.solve(torch.from_numpy(a[None]).cuda(), torch.from_numpy(b[None]).cuda())
        torch.cuda.synchronize()
        assert st.cpu().numpy().tolist() == want_st.tolist() == [OK], c
        infs += _assert_solve(x.cpu().numpy()[0], want[0], ("solve", c))
    assert infs >= 3


@DTYPES
def test_solve_ragged(solve_dll, inv_default, dtype):
    cs, mats, bs = _solve_systems(dtype)
    want = [mirror_solve(solve_dll, a, b) for a, b in zip(mats, bs)]
    assert [s for _, s in want] == [OK] * len(cs)
    orders, flat = pack(mats)
    plan = inv_default.plan_ragged(orders)
    try:
        x, st = inv_default.solve_ragged(plan, torch.from_numpy(flat).cuda(), torch.from_numpy(np.concatenate(bs)).cuda())
        torch.cuda.synchronize()
    finally:
        plan.close()
    assert st.cpu().numpy().tolist() == [OK] * len(cs)
    x = x.cpu().numpy()
    off = np.concatenate(([0], np.cumsum(orders)))
    infs = sum(_assert_solve(x[off[m]:off[m + 1]], want[m][0], ("solve_ragged", c)) for m, c in enumerate(cs))
    assert infs >= 3


# ---- host-pointer entry points -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,fn", [("host32", "matrix_inv_32"), ("host64", "matrix_inv_64"),
                                      ("host_nopivot", "matrix_inversion_no_pivots")])
def test_host_entry_points(oracle, route, fn):
    """Status 0: the reference's pattern comes back, never the empty vector of an invalid matrix."""
    ref, cases = C.ROUTES[route]
    for c in cases:
        want, st = C.reference(oracle, c, ref, 128 if ref == "mirror64" else None)   # the host call: the default width
        assert st == OK
        got = getattr(g, fn)(C.matrix(c).reshape(-1), c.n)
        assert got.shape == (c.n * c.n,), (fn, c, got.shape)
        assert_same(got.reshape(c.n, c.n), want, (fn, c))


# ---- the residual verifier ---------------------------------------------------------------------------------------------
def _cls(v):
    return "nan" if np.isnan(v) else "inf" if np.isinf(v) else "finite"


@pytest.mark.parametrize("c", cases_of("residual"))
def test_device_residual_of_an_overflowed_inverse(oracle, inv_blocked, c):
    """Both norms of an X that holds infinities and NaN are non-finite, in the class (inf or NaN) the oracle's double
    accumulation gives, never a finite number."""
    a, (x, _) = C.matrix(c), C.reference(oracle, c, "through")
    assert np.isinf(x).sum() >= 4 and np.isnan(x).any()
    r = inv_blocked.residual(torch.from_numpy(a).cuda(), torch.from_numpy(np.array(x)).cuda()).cpu().numpy()[0]
    want = (oracle.residual_inf(a, x, c.n), oracle.residual_inf_left(a, x, c.n))
    assert [_cls(v) for v in want].count("finite") == 0
    assert [_cls(v) for v in r[:2]] == [_cls(v) for v in want], (r, want)
