"""GPU tests of every inversion path on gradual underflow: subnormal inputs, subnormal steps and subnormal results (run
with ``-m gpu`` on an MI355X).  The inputs and the route table are those of tests/subnormal_cases.py;
tests/test_subnormal_cases.py proves on the CPU that the oracle and the mirrors give status 0 and a finite result for
every one of them, with the stated share of subnormal values.

There is no tolerance anywhere in this file but in the residual verifier's test, which keeps the ``rel=1e-9`` of
tests/test_gpu_parity.py.  A status is compared with the oracle's; a result byte for byte with the oracle's or the
mirror's, -0.0 stored as +0.0 (``canon``: conftest.canonical_bytes, kept in the member's dtype).  Every test body also
asserts ``share_subnormal`` of what it compared, so that a case that stopped being subnormal fails instead of passing
quietly.  No order above 640: no shared-panel or look-ahead geometry here.
"""
import numpy as np
import pytest

import subnormal_cases as C
from batch_helpers import strided
from degenerate_cases import canon
from det_cases import build_mirror, expected, same_doubles
from resident_cases import run
from solve_cases import build_solve_mirror, cap, mirror_solve, mirror_solve_batch
from vbatch_cases import pack, unpack

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_matrix_inversion_amd as g  # noqa: E402

F32, F64 = np.float32, np.float64
DTYPES = pytest.mark.parametrize("dtype", [F32, F64], ids=["fp32", "fp64"])
PIVOTING = pytest.mark.parametrize("pivoting", [True, False], ids=["pivot", "nopivot"])
OK = 0

_WANT = {}


def step_oracle(oracle, a, family, key=None):
    """(inverse (n, n), status) of the step-by-step oracle for this family and dtype; computed once per ``key`` and left
    unchanged."""
    if key is not None and key in _WANT:
        return _WANT[key]
    n = a.shape[0]
    if family.startswith("np_"):
        fn = oracle.matrix_inversion_no_pivots
    else:
        fn = oracle.matrix_inv_32_inplace if a.dtype == F32 else oracle.matrix_inv_64
    x, info = fn(a, n, return_info=True)
    x = x.reshape(n, n)
    x.setflags(write=False)
    if key is not None:
        _WANT[key] = (x, int(info["status"]))
    return x, int(info["status"])


def case(oracle, family, n, dtype):
    """(input, expected inverse) of a route-table case, the status asserted to be 0."""
    a = C.matrix(family, n, dtype)
    want, st = step_oracle(oracle, a, family, (family, n, dtype))
    assert st == OK == g.MI32_OK
    return a, want


def first_difference(got, want):
    """Where two results first differ (row-major) and both bit patterns: what a failure here is located by."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want).reshape(np.shape(got))
    u = np.uint32 if got.dtype == F32 else np.uint64
    bad = np.argwhere(got.view(u) != want.view(u))
    if not len(bad):
        return None
    i = tuple(int(v) for v in bad[0])
    return {"differing": len(bad), "first": i, "got": hex(int(got.view(u)[i])), "want": hex(int(want.view(u)[i]))}


def assert_same(got, want, tag):
    assert got.dtype == want.dtype and canon(got) == canon(want), (tag, first_difference(got, want))


def assert_subnormal(family, a, x, tag):
    """The input of a down family, the compared output of an up family."""
    side = a if family.endswith("down") else x
    assert C.share_subnormal(side) >= C.MIN_SHARE, (tag, family, C.share_subnormal(side))


def check_case(oracle, inv, family, n, dtype, tag, want=None):
    a, step = case(oracle, family, n, dtype)
    want = step if want is None else want
    got, st = run(inv, a)
    assert st.tolist() == [OK], (tag, family, n, st)
    assert_same(got, want, (tag, family, n))
    assert_subnormal(family, a, got, (tag, n))
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
inv_resident = _inverter_fixture(algo="resident")
inv_auto_nopivot = _inverter_fixture(algo="auto", pivoting=False)
inv_default = _inverter_fixture()
inv_default_nopivot = _inverter_fixture(pivoting=False)


@pytest.fixture(scope="module")
def one_launch():
    """{pivoting: handle}: ``algo="workgroup"`` takes the register-resident kernels up to 64 rows and the
    workgroup-resident ones above."""
    invs = {p: g.Inverter(algo="workgroup", pivoting=p) for p in (True, False)}
    yield invs
    for inv in invs.values():
        inv.close()


@pytest.fixture(scope="module")
def det_dll(tmp_path_factory):
    return build_mirror(tmp_path_factory.mktemp("det_mirror"))


@pytest.fixture(scope="module")
def solve_dll(tmp_path_factory):
    return build_solve_mirror(tmp_path_factory.mktemp("solve_mirror"))


# ---- fp32: sweep, blocked, no-pivot ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,n,family", C.cases("sweep32") + C.cases("sweep64"))
def test_sweep(oracle, inv_sweep, dtype, n, family):
    assert inv_sweep.resolved_algo(n, 1) == g.ALGO_SWEEP and inv_sweep.resolved_blocking_f64(n) == 0
    check_case(oracle, inv_sweep, family, n, dtype, "sweep")


@pytest.mark.parametrize("dtype,n,family", C.cases("blocked32"))
def test_blocked_fp32_default_plan(oracle, inv_blocked, dtype, n, family):
    assert inv_blocked.resolved_algo(n, 1) == g.ALGO_BLOCKED
    got = check_case(oracle, inv_blocked, family, n, dtype, "blocked")
    # above 300 rows the other GPU files take the oracle's cache-blocked evaluation: the same bits
    x, info = oracle.matrix_inv_32_blocked_exact(C.matrix(family, n, dtype), n, 128, return_info=True)
    assert info["status"] == OK and canon(got) == canon(x), (family, n)


@pytest.mark.parametrize("n,w", C.BLOCKED32_BW128)
def test_blocked_fp32_three_and_five_outer_blocks(oracle, n, w):
    """block_width = 128: rank-bw updates on the matrix cores with subnormal multipliers as the A operand (down) and with
    subnormal finished columns as C / D (up), at a narrow and at a wide sub-panel."""
    inv = g.Inverter(algo="blocked", panel_width=w, block_width=128)
    try:
        assert inv.resolved_algo(n, 1) == g.ALGO_BLOCKED and inv.resolved_blocking(n, 1) == (w, 128)
        widths = inv.resolved_panel_widths(n, 1)
        assert len(widths) == -(-n // 128) == {300: 3, 640: 5}[n] and widths[0] == w
        for dtype, order, family in C.cases("blocked32_bw128"):
            if order == n:
                check_case(oracle, inv, family, n, dtype, ("blocked bw 128", w))
    finally:
        inv.close()


def test_blocked_fp32_batch(oracle, inv_blocked):
    n, fams = C.BLOCKED32_BATCH
    mats, names = C.mixed_members([n] * len(fams), F32, fams)
    assert inv_blocked.resolved_algo(n, len(mats)) == g.ALGO_BLOCKED
    want = [step_oracle(oracle, a, nm) for a, nm in zip(mats, names)]
    got, st = run(inv_blocked, np.stack(mats))
    assert st.tolist() == [s for _, s in want] == [OK] * len(mats)
    for b, (a, nm) in enumerate(zip(mats, names)):
        assert_same(got[b], want[b][0], ("blocked batch", b, nm))
        if nm != "gate":
            assert_subnormal(nm, a, got[b], ("blocked batch", b))


@pytest.mark.parametrize("dtype,n,family", C.cases("nopivot32_sweep") + C.cases("nopivot32_blocked")
                         + C.cases("nopivot64_sweep") + C.cases("nopivot64_blocked"))
def test_no_pivot_sweep_and_blocked(oracle, inv_auto_nopivot, dtype, n, family):
    """Below 512 rows the sweep, from there the blocked fp32 path in its no-pivot shape and mi32_nopivot64.hip: all
    against the step-by-step no-pivot oracle."""
    inv = inv_auto_nopivot
    blocked = n >= 512
    if dtype == F32:
        assert inv.resolved_algo(n, 1) == (g.ALGO_BLOCKED if blocked else g.ALGO_SWEEP)
    else:
        assert (inv.resolved_blocking_f64(n) > 0) == blocked
    check_case(oracle, inv, family, n, dtype, "no pivot")


# ---- fp64 blocked ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bw_req", [0, 64])
@pytest.mark.parametrize("dtype,n,family", C.cases("blocked64"))
def test_blocked_fp64(oracle, dtype, n, family, bw_req):
    """Against the fp64 blocked mirror at the width the plan reports: rank-bw updates on v_mfma_f64_16x16x4_f64."""
    inv = g.Inverter(algo="auto", block_width=bw_req)
    try:
        bw = inv.resolved_blocking_f64(n)
        assert bw in C.F64_BLOCKED_WIDTHS and (bw_req == 0 or bw == bw_req)
        a = C.matrix(family, n, dtype)
        want, info = oracle.matrix_inv_64_blocked(a, n, bw, return_info=True)
        assert info["status"] == OK
        check_case(oracle, inv, family, n, dtype, ("blocked fp64", bw), want=want.reshape(n, n))
    finally:
        inv.close()


# ---- resident and workgroup ------------------------------------------------------------------------------------------
def _check_mixed_batch(oracle, inv, mats, names, tag):
    """One uniform call on a batch that alternates the two subnormal families and an ordinary member."""
    want = [step_oracle(oracle, a, nm) for a, nm in zip(mats, names)]
    got, st = run(inv, mats)
    assert got.dtype == mats.dtype and st.tolist() == [s for _, s in want] == [OK] * len(mats), (tag, st)
    sides = {}
    for b, (a, nm) in enumerate(zip(mats, names)):
        assert_same(got[b], want[b][0], (tag, b, nm))
        sides.setdefault(nm, []).append((a if nm.endswith("down") else got[b]).reshape(-1))
    assert len(sides) == 3, tag
    for nm, parts in sides.items():
        if nm not in ("gate", "np_plain"):
            assert C.share_subnormal(np.concatenate(parts)) >= C.MIN_SHARE, (tag, nm)
    return got


@DTYPES
@PIVOTING
@pytest.mark.parametrize("n", C.RESIDENT_ORDERS)
def test_resident_mixed_batch(oracle, one_launch, inv_resident, n, pivoting, dtype):
    inv = one_launch[pivoting]
    assert inv.resolved_algo(n, C.RESIDENT_BATCH) == g.ALGO_RESIDENT
    mats, names = C.mixed_batch(n, C.RESIDENT_BATCH, dtype, C.batch_families(pivoting))
    got = _check_mixed_batch(oracle, inv, mats, names, ("resident", n, pivoting))
    if pivoting:           # and through algo="resident" itself
        assert inv_resident.resolved_algo(n, C.RESIDENT_BATCH) == g.ALGO_RESIDENT
        again, st = run(inv_resident, mats)
        assert not st.any() and again.tobytes() == got.tobytes()


@DTYPES
@PIVOTING
@pytest.mark.parametrize("n", C.WORKGROUP_ORDERS)
def test_workgroup_mixed_batch(oracle, one_launch, n, pivoting, dtype):
    inv = one_launch[pivoting]
    assert inv.resolved_algo(n, C.WORKGROUP_BATCH) == g.ALGO_WORKGROUP
    mats, names = C.mixed_batch(n, C.WORKGROUP_BATCH, dtype, C.batch_families(pivoting))
    _check_mixed_batch(oracle, inv, mats, names, ("workgroup", n, pivoting))


# ---- mixed orders in one call ----------------------------------------------------------------------------------------
def _ragged_members(oracle, dtype):
    mats, names = C.mixed_members(C.RAGGED_ORDERS * C.RAGGED_COPIES, dtype, C.batch_families(True))
    want = [step_oracle(oracle, a, nm, ("ragged", b, dtype)) for b, (a, nm) in enumerate(zip(mats, names))]
    assert [s for _, s in want] == [OK] * len(mats)
    return mats, names, [x for x, _ in want]


def _assert_ragged(got, mats, names, want, tag):
    sides = {}
    for b, (a, nm) in enumerate(zip(mats, names)):
        assert_same(np.ascontiguousarray(got[b]), want[b], (tag, b, nm, a.shape[0]))
        sides.setdefault(nm, []).append((a if nm.endswith("down") else np.asarray(got[b])).reshape(-1))
    for nm in ("down", "up"):
        assert C.share_subnormal(np.concatenate(sides[nm])) >= C.MIN_SHARE, (tag, nm)


@DTYPES
def test_ragged_call_packed(oracle, inv_default, dtype):
    mats, names, want = _ragged_members(oracle, dtype)
    orders, flat = pack(mats)
    plan = inv_default.plan_ragged(orders)
    try:
        x, st = inv_default.inv_ragged(plan, torch.from_numpy(flat).cuda())
        torch.cuda.synchronize()
    finally:
        plan.close()
    assert st.cpu().numpy().tolist() == [OK] * len(mats)
    _assert_ragged(unpack(x.cpu().numpy(), orders), mats, names, want, "ragged")


@DTYPES
def test_ragged_call_strided_between_nan_padding(oracle, inv_default, dtype):
    mats, names, want = _ragged_members(oracle, dtype)
    tdt, es = (torch.float32, 4) if dtype == F32 else (torch.float64, 8)
    sentinel = dtype(-12345.5)
    a_buf, a_off, lda, _ = strided(mats, 3, np.nan)            # NaN in the input padding: never read
    o_buf, o_off, ldo, o_pad = strided([np.zeros_like(m) for m in mats], 5, sentinel)
    o_buf[:] = sentinel
    ta, to = torch.from_numpy(a_buf).cuda(), torch.from_numpy(o_buf).cuda()
    plan = inv_default.plan_ragged([m.shape[0] for m in mats])
    try:
        st = inv_default.inv_pointers(plan, torch.from_numpy(a_off * es + ta.data_ptr()).cuda(),
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
    _assert_ragged(got, mats, names, want, "strided")


# ---- the determinant beside the inverse ------------------------------------------------------------------------------
def _det_members(orders, dtype, pivoting):
    fams = C.ROUTES["det" if pivoting else "det_nopivot"][2]
    mats, names = [], []
    for n in orders:
        for fam in fams:
            mats.append(C.matrix(fam, n, dtype))
            names.append(fam)
    return mats, names


def _assert_det(x, st, mant, exp, plain, mats, names, want, tag):
    """Mantissa and exponent against the mirror's recurrence, inverse and status against the mirror and against the
    plain call's bits; ``down`` is the case that matters: subnormal pivots into frexp, exponents near E n."""
    want_x, want_st, want_m, want_e = want
    assert np.array_equal(st, want_st) and not st.any(), (tag, st)
    for b, (a, nm) in enumerate(zip(mats, names)):
        n = a.shape[0]
        assert_same(np.ascontiguousarray(x[b]), want_x[b], (tag, n, nm))
        assert np.ascontiguousarray(x[b]).tobytes() == np.ascontiguousarray(plain[b]).tobytes(), (tag, n, nm, "plain call")
        assert same_doubles(mant[b:b + 1], want_m[b:b + 1]) and exp[b] == want_e[b], \
            (tag, n, nm, float(mant[b]).hex(), float(want_m[b]).hex(), int(exp[b]), int(want_e[b]))
        assert 0.5 <= abs(mant[b]) < 1.0 and abs(int(exp[b]) - C.exponent(nm, a.dtype, n) * n) <= 6 * n, (tag, n, nm)
        assert_subnormal(nm, a, np.asarray(x[b]), (tag, n))


@DTYPES
@PIVOTING
def test_inv_det_uniform(det_dll, inv_default, inv_default_nopivot, pivoting, dtype):
    inv = inv_default if pivoting else inv_default_nopivot
    for n in C.ROUTES["det"][1]:
        mats, names = _det_members([n], dtype, pivoting)
        batch = np.stack(mats)
        want = expected(det_dll, mats, pivoting)
        x, st, mant, exp = inv.inv_det(torch.from_numpy(batch).cuda())
        plain, plain_st = inv.inv(torch.from_numpy(batch).cuda())
        torch.cuda.synchronize()
        assert torch.equal(st, plain_st)
        _assert_det(x.cpu().numpy(), st.cpu().numpy(), mant.cpu().numpy(), exp.cpu().numpy(), plain.cpu().numpy(), mats,
                    names, want, ("inv_det", pivoting))


@DTYPES
@PIVOTING
def test_inv_ragged_with_det(det_dll, inv_default, inv_default_nopivot, pivoting, dtype):
    inv = inv_default if pivoting else inv_default_nopivot
    mats, names = _det_members(C.ROUTES["det"][1], dtype, pivoting)
    want = expected(det_dll, mats, pivoting)
    orders, flat = pack(mats)
    plan = inv.plan_ragged(orders)
    try:
        tf = torch.from_numpy(flat).cuda()
        x, st, (mant, exp) = inv.inv_ragged(plan, tf, det=True)
        plain, plain_st = inv.inv_ragged(plan, tf)
        torch.cuda.synchronize()
    finally:
        plan.close()
    assert torch.equal(st, plain_st)
    _assert_det(unpack(x.cpu().numpy(), orders), st.cpu().numpy(), mant.cpu().numpy(), exp.cpu().numpy(),
                unpack(plain.cpu().numpy(), orders), mats, names, want, ("inv_ragged det", pivoting))


# ---- A X = B ---------------------------------------------------------------------------------------------------------
def _assert_solve(family, a, b, x, want, tag):
    assert x.dtype == want.dtype and np.array_equal(x, want), (tag, family, first_difference(x, want))
    if family == "down":          # A and B subnormal, X ordinary
        assert C.share_subnormal(a) >= C.MIN_SHARE and C.share_subnormal(b) >= 0.99, tag
    else:                         # X subnormal
        assert C.share_subnormal(x) >= C.MIN_SHARE_SOLVE_UP, (tag, C.share_subnormal(x))


@DTYPES
def test_solve(solve_dll, inv_default, dtype):
    in_place_done = False
    for n, k in C.solve_shapes():
        assert inv_default.resolved_solve(n, k)[1] == -(-k // cap(n)) and (k == C.SOLVE_K or k == cap(n) + 1)
        mats = np.stack([C.matrix(fam, n, dtype) for fam in C.PIVOTED])
        rhs = np.stack([C.solve_rhs(fam, n, k, dtype) for fam in C.PIVOTED])
        want, want_st = mirror_solve_batch(solve_dll, mats, rhs)
        ta, tb = torch.from_numpy(mats).cuda(), torch.from_numpy(rhs).cuda()
        x, st = inv_default.solve(ta, tb)
        torch.cuda.synchronize()
        assert st.cpu().numpy().tolist() == want_st.tolist() == [OK, OK], (n, k)
        x = x.cpu().numpy()
        for m, fam in enumerate(C.PIVOTED):
            _assert_solve(fam, mats[m], rhs[m], x[m], want[m], ("solve", n, k))
        if n == 100 and k == C.SOLVE_K and not in_place_done:      # the in-place form, once per dtype
            x2, st2 = inv_default.solve(ta, tb, out=tb)
            torch.cuda.synchronize()
            assert x2.data_ptr() == tb.data_ptr() and not st2.any().item()
            assert np.array_equal(tb.cpu().numpy(), x)
            in_place_done = True
    assert in_place_done


@DTYPES
@pytest.mark.parametrize("k", list(C.SOLVE_RAGGED), ids=["K3", "two-chunks-at-100"])
def test_solve_ragged(solve_dll, inv_default, dtype, k):
    orders = list(C.SOLVE_RAGGED[k]) * 2
    fams = [C.PIVOTED[b // len(C.SOLVE_RAGGED[k])] for b in range(len(orders))]
    mats = [C.matrix(f, n, dtype) for f, n in zip(fams, orders)]
    bs = [C.solve_rhs(f, n, k, dtype) for f, n in zip(fams, orders)]
    want = [mirror_solve(solve_dll, a, b) for a, b in zip(mats, bs)]
    assert [s for _, s in want] == [OK] * len(mats)
    _, flat = pack(mats)
    plan = inv_default.plan_ragged(orders)
    try:
        x, st = inv_default.solve_ragged(plan, torch.from_numpy(flat).cuda(), torch.from_numpy(np.concatenate(bs)).cuda())
        torch.cuda.synchronize()
    finally:
        plan.close()
    assert st.cpu().numpy().tolist() == [OK] * len(mats)
    x = x.cpu().numpy()
    off = np.concatenate(([0], np.cumsum(orders)))
    for m, fam in enumerate(fams):
        _assert_solve(fam, mats[m], bs[m], x[off[m]:off[m + 1]], want[m][0], ("solve_ragged", orders[m], k))


# ---- host-pointer entry points ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,fn", [("host32", "matrix_inv_32"), ("host64", "matrix_inv_64"),
                                      ("host_nopivot", "matrix_inversion_no_pivots")])
def test_host_entry_points(oracle, route, fn):
    for dtype, n, family in C.cases(route):
        a, want = case(oracle, family, n, dtype)
        if route == "host64":       # from N = 256 on the host call takes the blocked fp64 path: its mirror at the default width
            x, info = oracle.matrix_inv_64_blocked(a, n, 128, return_info=True)
            assert info["status"] == OK
            want = x.reshape(n, n)
        got = getattr(g, fn)(a.reshape(-1), n)
        assert got.shape == (n * n,), (fn, family, got.shape)
        got = got.reshape(n, n)
        assert_same(got, want, (fn, family, n))
        assert_subnormal(family, a, got, (fn, n))


# ---- the residual verifier -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,n,family", C.cases("residual"))
def test_device_residual_of_subnormal_operands(oracle, inv_blocked, dtype, n, family):
    """``up``: a huge A with its subnormal inverse; ``down``: a subnormal A with its huge inverse -- the verifier's
    fp32 -> fp64 conversions of subnormal values, against the oracle's double accumulation."""
    a, x = case(oracle, family, n, dtype)
    assert_subnormal(family, a, x, ("residual", n))
    r = inv_blocked.residual(torch.from_numpy(a).cuda(), torch.from_numpy(np.array(x)).cuda()).cpu().numpy()[0]
    assert r[0] == pytest.approx(oracle.residual_inf(a, x, n), rel=1e-9)
    assert r[1] == pytest.approx(oracle.residual_inf_left(a, x, n), rel=1e-9)


# ---- output overflow -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["sweep", "blocked", "resident"])
@pytest.mark.parametrize("n", C.OVERFLOW_OUT_ORDERS)
def test_output_overflow_keeps_status_0(oracle, inv_sweep, inv_blocked, inv_resident, n, path):
    """Every pivot is finite, so the status is 0 -- it looks at pivots and input entries only -- while the inverse
    overflows: the same non-finite positions as the oracle (infinities with their sign, NaN as one value) and the
    finite entries bit for bit.

    The blocked path is the one that can get this wrong: it pads to 128 rows with an identity block and multiplies zero
    multipliers through, so a padded row takes fmaf(-0, +-inf, 0) = NaN wherever a pivot row holds an infinity.  With
    the padding behind the matrix the padded rows' own steps carried those NaNs back into every real row of the column
    (n = 16: columns 4 and 15 wholly NaN where the oracle holds +-inf in 10 and 16 of their entries); the padding now
    comes first and its rows are retired before the first real step."""
    inv = {"sweep": inv_sweep, "blocked": inv_blocked, "resident": inv_resident}[path]
    assert inv.resolved_algo(n, 1) == {"sweep": g.ALGO_SWEEP, "blocked": g.ALGO_BLOCKED, "resident": g.ALGO_RESIDENT}[path]
    a = C.overflow_out(n)
    want, info = oracle.matrix_inv_32_inplace(a, n, return_info=True)
    assert info["status"] == OK and not np.isfinite(want).all() and C.share_subnormal(a) >= C.MIN_SHARE
    got, st = run(inv, a)
    assert st.tolist() == [OK], (path, n, st)
    assert C.same_with_nonfinite(got, want), (path, n, got.reshape(-1)[:8], want[:8])
