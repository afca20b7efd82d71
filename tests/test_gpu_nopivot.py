"""GPU tests of the no-pivot variant (``pivoting=False``, the reference's matrix_inversion_no_pivots) on inputs that are
NOT diagonally dominant (tests/nopivot_cases.py; tests/test_nopivot_cases.py proves them on the CPU oracle): every
device implementation of it -- the fp32 and fp64 sweep kernels, the register-resident and workgroup-resident kernels
with their solve, determinant and variable-size twins, the fp32 blocked path in its no-pivot shape and the blocked fp64
path of mi32_nopivot64.hip.  Run with ``-m gpu`` on an MI355X.

There is no tolerance anywhere in this file.  A valid result is compared with the oracle's no-pivot result of the same
matrix: ``np.array_equal`` on the sweep, resident and workgroup kernels, byte for byte with -0.0 stored as +0.0
(``degenerate_cases.canon``) on the two blocked paths, which multiply zero multipliers through.  A status is compared
with the oracle's and with the literal constant; a flagged member's values are never looked at.
"""
import numpy as np
import pytest

import nopivot_cases as C
from degenerate_cases import canon
from det_cases import build_mirror, expected, same_doubles
from resident_cases import run
from solve_cases import build_solve_mirror, mirror_solve_batch, rhs
from vbatch_cases import pack, unpack

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_matrix_inversion_amd as g  # noqa: E402

DTYPES = [np.float32, np.float64]
IDS = ["fp32", "fp64"]
ONE_LAUNCH_ORDERS = C.RESIDENT_ORDERS + C.WORKGROUP_ORDERS

_ORACLE = {}


def oracle_of(oracle, a, key=None):
    """(flat inverse, status) of the oracle's no-pivot restatement; computed once per ``key`` and left unchanged."""
    if key is not None and key in _ORACLE:
        return _ORACLE[key]
    n = a.shape[0]
    x, info = oracle.matrix_inversion_no_pivots(a, n, return_info=True)
    assert x.dtype == a.dtype
    x.setflags(write=False)
    if key is not None:
        _ORACLE[key] = (x, int(info["status"]))
    return x, int(info["status"])


def want_of(oracle, name, n, dtype):
    """The oracle's inverse of family ``name``, whose status is 0."""
    x, st = oracle_of(oracle, C.family(name, n, dtype), (name, n, dtype))
    assert st == C.STATUS_OK == g.MI32_OK
    return x


def members_of(oracle, mats):
    outs = []
    for a in mats:
        x, st = oracle_of(oracle, a)
        assert st == C.STATUS_OK
        outs.append(x.reshape(a.shape))
    return outs


def check_families(oracle, inv, n, dtype, same, names=C.FAMILIES, tag=None):
    """Every family at order n through ``inv``: status 0 and the oracle's inverse under the comparison ``same``; then
    the two identities that hold bit for bit, on the device's own results."""
    got = {}
    for name in names:
        x, st = run(inv, C.family(name, n, dtype))
        assert x.dtype == dtype and st.tolist() == [C.STATUS_OK], (tag, name, n, st)
        assert same(x.reshape(-1), want_of(oracle, name, n, dtype)), (tag, name, n)
        got[name] = x
    seed = C.seed_of(n)
    if "spd" in got and "spd_scaled" in got:      # inv(D a D) = D^-1 inv(a) D^-1: scaling by powers of two is exact
        assert same(C.unscale(got["spd_scaled"], n, seed, dtype), got["spd"]), (tag, "scaling identity", n)
    if "spd" in got and "spd_signed" in got:      # negated rows: the same inverse with those columns negated
        flipped = got["spd"].copy()
        flipped[:, C.negated_rows(n, seed)] *= -1
        assert same(got["spd_signed"], flipped), (tag, "sign identity", n)
    return got


def same_canon(x, y):
    return x.dtype == y.dtype and canon(x) == canon(y)


def same_values(x, y):
    return x.dtype == y.dtype and np.array_equal(np.asarray(x).reshape(-1), np.asarray(y).reshape(-1))


@pytest.fixture(scope="module")
def inv_auto():
    i = g.Inverter(algo="auto", pivoting=False)
    yield i
    i.close()


@pytest.fixture(scope="module")
def inv_one_launch():
    """``algo="workgroup"`` takes the register-resident kernels up to 64 rows and the workgroup-resident ones above."""
    i = g.Inverter(algo="workgroup", pivoting=False)
    yield i
    i.close()


@pytest.fixture(scope="module")
def inv_default():
    i = g.Inverter(pivoting=False)
    yield i
    i.close()


@pytest.fixture(scope="module")
def solve_dll(tmp_path_factory):
    return build_solve_mirror(tmp_path_factory.mktemp("solve_mirror"))


@pytest.fixture(scope="module")
def det_dll(tmp_path_factory):
    return build_mirror(tmp_path_factory.mktemp("det_mirror"))


# ---- fp32 blocked ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.BLOCKED32_ORDERS)
def test_blocked_fp32_families(oracle, inv_auto, n):
    assert inv_auto.resolved_algo(n, 1) == g.ALGO_BLOCKED
    check_families(oracle, inv_auto, n, np.float32, same_canon, tag="blocked fp32")


@pytest.mark.parametrize("n", C.BLOCKED32_EXPLICIT_ORDERS)
def test_blocked_fp32_explicit_below_the_cross_over(oracle, n):
    inv = g.Inverter(algo="blocked", pivoting=False)
    try:
        assert inv.resolved_algo(n, 1) == g.ALGO_BLOCKED
        check_families(oracle, inv, n, np.float32, same_canon, tag="explicit blocked fp32")
    finally:
        inv.close()


@pytest.mark.parametrize("bw", C.BLOCKED32_WIDTHS)
def test_blocked_fp32_outer_block_widths(oracle, bw):
    n = 1000
    inv = g.Inverter(algo="auto", pivoting=False, block_width=bw)
    try:
        assert inv.resolved_algo(n, 1) == g.ALGO_BLOCKED and inv.resolved_blocking(n)[1] == bw
        check_families(oracle, inv, n, np.float32, same_canon, names=("spd_scaled", "sparse_spd"), tag=f"bw {bw}")
    finally:
        inv.close()


def test_blocked_fp32_lookahead_forced_on(oracle, monkeypatch):
    """The look-ahead schedule (its default starts above 4096 rows) on spd_scaled at n = 2048, then the single-stream
    schedule: the oracle's result, and the two equal bit for bit."""
    n = C.LOOKAHEAD_ORDER
    a = C.family("spd_scaled", n, np.float32)
    want = want_of(oracle, "spd_scaled", n, np.float32)
    monkeypatch.setenv("MI32_LOOKAHEAD_MIN", str(n))   # read per call
    inv = g.Inverter(algo="auto", pivoting=False)
    try:
        assert inv.resolved_algo(n, 1) == g.ALGO_BLOCKED and inv.resolved_route(n)[0]["lookahead"] == 1
        ta = torch.from_numpy(a).cuda()
        x, st = inv.inv(ta)
        torch.cuda.synchronize()
        assert st.tolist() == [C.STATUS_OK] and same_canon(x.cpu().numpy().reshape(-1), want)
        inv.set_lookahead(False)
        assert inv.resolved_route(n)[0]["lookahead"] == 0
        x1, st1 = inv.inv(ta)
        torch.cuda.synchronize()
        assert st1.tolist() == [C.STATUS_OK] and x1.cpu().numpy().tobytes() == x.cpu().numpy().tobytes()
    finally:
        inv.close()


# ---- fp64 blocked (mi32_nopivot64.hip) ------------------------------------------------------------------------------
@pytest.mark.parametrize("bw", C.BLOCKED64_WIDTHS)
@pytest.mark.parametrize("n", C.BLOCKED64_ORDERS)
def test_blocked_fp64_families(oracle, n, bw):
    inv = g.Inverter(algo="auto", pivoting=False, block_width=bw)
    try:
        assert inv.resolved_blocking_f64(n) == bw
        check_families(oracle, inv, n, np.float64, same_canon, tag=f"blocked fp64 bw {bw}")
    finally:
        inv.close()


@pytest.mark.parametrize("bw", C.BLOCKED64_WIDTHS)
@pytest.mark.parametrize("n", C.BLOCKED64_EXPLICIT_ORDERS)
def test_blocked_fp64_explicit_below_the_cross_over(oracle, n, bw):
    inv = g.Inverter(algo="blocked", pivoting=False, block_width=bw)
    try:
        assert inv.resolved_blocking_f64(n) == bw
        check_families(oracle, inv, n, np.float64, same_canon, tag=f"explicit blocked fp64 bw {bw}")
    finally:
        inv.close()


# ---- sweep ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", C.SWEEP_ORDERS)
def test_sweep_families(oracle, n, dtype):
    inv = g.Inverter(algo="sweep", pivoting=False)
    try:
        assert inv.resolved_algo(n, 1) == g.ALGO_SWEEP and inv.resolved_blocking_f64(n) == 0
        check_families(oracle, inv, n, dtype, same_values, tag="sweep")
    finally:
        inv.close()


# ---- resident and workgroup: inverse, variable-size, solve, determinant ---------------------------------------------
def expected_algo(n):
    return g.ALGO_RESIDENT if n <= 64 else g.ALGO_WORKGROUP


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", ONE_LAUNCH_ORDERS)
def test_one_launch_families_side_by_side(oracle, inv_one_launch, n, dtype):
    mats, names, seeds = C.side_by_side(n, dtype)
    assert inv_one_launch.resolved_algo(n, len(mats)) == expected_algo(n)
    want = members_of(oracle, mats)
    got, st = run(inv_one_launch, mats)
    assert got.dtype == dtype and st.tolist() == [C.STATUS_OK] * len(mats)
    for b in range(len(mats)):
        assert np.array_equal(got[b], want[b]), (names[b], n, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_launch_every_order_in_one_plan(oracle, inv_one_launch, dtype):
    mats, names = [], []
    for n in ONE_LAUNCH_ORDERS:
        m, nm, _ = C.side_by_side(n, dtype)
        mats += list(m)
        names += nm
    order = np.random.default_rng(2).permutation(len(mats))
    mats, names = [mats[i] for i in order], [names[i] for i in order]
    want = members_of(oracle, mats)
    orders, flat = pack(mats)
    plan = inv_one_launch.plan_ragged(orders)
    try:
        x, st = inv_one_launch.inv_ragged(plan, torch.from_numpy(flat).cuda())
        torch.cuda.synchronize()
    finally:
        plan.close()
    assert st.cpu().numpy().tolist() == [C.STATUS_OK] * len(mats)
    got = unpack(x.cpu().numpy(), orders)
    for b in range(len(mats)):
        assert got[b].dtype == dtype and np.array_equal(got[b], want[b]), (names[b], mats[b].shape[0], b)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_launch_solve(solve_dll, inv_default, dtype):
    for n in ONE_LAUNCH_ORDERS:
        if n > 127:
            continue
        mats, names, _ = C.side_by_side(n, dtype)
        for k in (1, 3):
            b = np.stack([rhs(n, k, 100 * n + 10 * k + m, dtype) for m in range(len(mats))])
            want_x, want_st = mirror_solve_batch(solve_dll, mats, b, pivoting=False)
            assert want_st.tolist() == [C.STATUS_OK] * len(mats)
            x, st = inv_default.solve(torch.from_numpy(mats).cuda(), torch.from_numpy(b).cuda())
            torch.cuda.synchronize()
            assert st.cpu().numpy().tolist() == [C.STATUS_OK] * len(mats), (n, k)
            x = x.cpu().numpy()
            for m in range(len(mats)):
                assert x.dtype == dtype and np.array_equal(x[m], want_x[m]), (names[m], n, k, m)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_launch_determinant_with_negative_pivots(oracle, det_dll, inv_default, dtype):
    """det = prod pivots with no swaps: the negated rows of spd_signed make about half of the pivots negative, so the
    mantissa's sign is (-1)^(negated rows) times spd's, and both signs occur."""
    signs = set()
    for n in ONE_LAUNCH_ORDERS:
        mats, names, seeds = C.side_by_side(n, dtype)
        want_x, want_st, want_m, want_e = expected(det_dll, mats, pivoting=False)
        assert want_st.tolist() == [C.STATUS_OK] * len(mats)
        x, st, mant, exp = inv_default.inv_det(torch.from_numpy(mats).cuda())
        torch.cuda.synchronize()
        x, st, mant, exp = x.cpu().numpy(), st.cpu().numpy(), mant.cpu().numpy(), exp.cpu().numpy()
        assert st.tolist() == [C.STATUS_OK] * len(mats), n
        for b, ox in enumerate(members_of(oracle, mats)):
            assert np.array_equal(x[b], ox) and np.array_equal(x[b], want_x[b]), (names[b], n, b)
        assert same_doubles(mant, want_m), (n, mant, want_m)
        assert np.array_equal(exp, want_e), (n, exp, want_e)
        assert (np.abs(mant) >= 0.5).all() and (np.abs(mant) < 1.0).all()
        for b in range(len(mats)):
            if names[b] == "spd_signed":
                base = next(c for c in range(len(mats)) if names[c] == "spd" and seeds[c] == seeds[b])
                flips = len(C.negated_rows(n, seeds[b]))
                assert mant[base] > 0 and np.sign(mant[b]) == (-1) ** flips, (n, b, flips, mant[b])
                assert abs(mant[b]) == mant[base] and exp[b] == exp[base], (n, b)   # the pivots' magnitudes are spd's
                signs.add(float(np.sign(mant[b])))
            else:
                assert mant[b] > 0, (names[b], n, b)                               # symmetric positive definite
    assert signs == {-1.0, 1.0}


# ---- bad pivots, late and on seams ----------------------------------------------------------------------------------
def zero_pivot_inverter(path, bw):
    if path == "blocked32" or path == "blocked64":
        return g.Inverter(algo="auto", pivoting=False, block_width=bw)
    return g.Inverter(algo={"sweep": "sweep", "resident": "workgroup", "workgroup": "workgroup"}[path], pivoting=False)


@pytest.mark.parametrize("path,dtype,n,bw,steps", C.ZERO_PIVOTS,
                         ids=[f"{p}-{np.dtype(d).name}-{n}-{bw}" for p, d, n, bw, _ in C.ZERO_PIVOTS])
def test_zero_pivot_is_status_2(oracle, path, dtype, n, bw, steps):
    base = C.family("spd", n, dtype)
    inv = zero_pivot_inverter(path, bw)
    try:
        if path == "blocked32":
            assert inv.resolved_algo(n, 1) == g.ALGO_BLOCKED
        elif path == "blocked64":
            assert inv.resolved_blocking_f64(n) == bw if bw else inv.resolved_blocking_f64(n) > 0
        elif path == "sweep":
            assert inv.resolved_algo(n, 1) == g.ALGO_SWEEP and inv.resolved_blocking_f64(n) == 0
        else:
            assert inv.resolved_algo(n, 4) == expected_algo(n)
        for k in steps:
            hit = C.zero_pivot_at(base, k)
            want = oracle_of(oracle, hit, ("zero", n, dtype, k))[1]
            _, st = run(inv, hit)
            assert st.tolist() == [want] == [C.STATUS_SINGULAR] == [g.MI32_SINGULAR], (path, n, k, st)
        if path in ("resident", "workgroup"):    # and between regular members, which keep the oracle's bits
            batch = np.stack([base, C.zero_pivot_at(base, steps[0]), base, C.zero_pivot_at(base, steps[1])])
            x, st = run(inv, batch)
            assert st.tolist() == [0, 2, 0, 2], (path, n, st)
            want = want_of(oracle, "spd", n, dtype)
            assert same_values(x[0], want) and same_values(x[2], want), (path, n)
    finally:
        inv.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_blocked_batch_with_a_flagged_member(oracle, inv_auto, dtype):
    """[spd, zero pivot at the last step, spd_scaled, near_cancellation] at n = 600 on the blocked path of the dtype:
    status [0, 2, 0, 0]; members 0, 2 and 3 have the oracle's bits and those of a single-matrix call; the next call
    on the same handle is clean."""
    n = C.BATCH_ORDER
    mats, want_st = C.status_batch(dtype)
    if dtype == np.float32:
        assert inv_auto.resolved_algo(n, len(mats)) == g.ALGO_BLOCKED
    else:
        assert inv_auto.resolved_blocking_f64(n) > 0
    oracles = [oracle_of(oracle, a, ("batch", dtype, b)) for b, a in enumerate(mats)]
    assert [st for _, st in oracles] == want_st == [0, 2, 0, 0]
    x, st = run(inv_auto, np.stack(mats))
    assert st.tolist() == want_st
    for b in (0, 2, 3):
        assert same_canon(x[b].reshape(-1), oracles[b][0]), b
        xs, sts = run(inv_auto, mats[b])
        assert sts.tolist() == [C.STATUS_OK] and same_canon(xs, x[b]), b
    xs, sts = run(inv_auto, mats[1])
    assert sts.tolist() == [C.STATUS_SINGULAR]
    xs, sts = run(inv_auto, mats[0])                  # the next call on the same handle is clean
    assert sts.tolist() == [C.STATUS_OK] and same_canon(xs.reshape(-1), oracles[0][0])


# ---- host entry points ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.HOST_ORDERS)
def test_host_entry_points(oracle, n):
    a = C.family("spd_scaled", n, np.float64)
    want = want_of(oracle, "spd_scaled", n, np.float64)
    got = g.matrix_inversion_no_pivots(a.reshape(-1), n)
    assert got.shape == (n * n,) and same_canon(got, want)
    y, times = g.fp64_bench(a.reshape(-1), n, pivoting=False)
    assert y.shape == (n * n,) and same_canon(y, want) and times["column"] > 0
    hit = C.zero_pivot_at(C.family("spd", n, np.float64), n - 1)
    assert oracle_of(oracle, hit, ("zero", n, np.float64, n - 1))[1] == C.STATUS_SINGULAR
    assert g.matrix_inversion_no_pivots(hit.reshape(-1), n).size == 0
    y, times = g.fp64_bench(hit.reshape(-1), n, pivoting=False)
    assert y.size == 0 and times == {}
