"""CPU-only proof that the inputs of tests/subnormal_cases.py are what they claim to be, for every entry of its route
table: the oracle (or the mirror the route is held to) gives status 0 and a wholly finite result, the input holds no
infinity, and at least a quarter of the input (down families) or of the expected output (up families) is subnormal
-- a fifth for the X of ``solve up``.  A precondition of tests/test_gpu_subnormal.py, not a measurement: the thresholds
are conditions the reference meets alone, and there is no tolerance anywhere."""
import numpy as np
import pytest

import subnormal_cases as C
from degenerate_cases import canon
from det_cases import build_mirror, expected, mirror
from solve_cases import build_solve_mirror, mirror_solve

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def det_dll(tmp_path_factory):
    return build_mirror(tmp_path_factory.mktemp("det_mirror"))


@pytest.fixture(scope="module")
def solve_dll(tmp_path_factory):
    return build_solve_mirror(tmp_path_factory.mktemp("solve_mirror"))


def step_oracle(oracle, a, family):
    """(inverse (n, n), status) of the step-by-step oracle for this family and dtype."""
    n = a.shape[0]
    if family in C.NOPIVOT or family == "np_plain":
        fn = oracle.matrix_inversion_no_pivots
    else:
        fn = oracle.matrix_inv_32_inplace if a.dtype == F32 else oracle.matrix_inv_64
    x, info = fn(a, n, return_info=True)
    assert x.dtype == a.dtype
    return x.reshape(n, n), int(info["status"])


def subnormal_side(family, a, x):
    """What must be subnormal: the input of a down family, the output of an up family."""
    return a if family.endswith("down") else x


def test_share_subnormal_counts_nonzero_values_below_the_smallest_normal():
    x = np.array([0.0, -0.0, 2.0 ** -126, -2.0 ** -127, 2.0 ** -149, 1.0, np.inf, np.nan], F32)
    assert C.share_subnormal(x) == 2 / 8
    y = np.array([2.0 ** -1022, 2.0 ** -1023, -2.0 ** -1074, 0.0], F64)
    assert C.share_subnormal(y) == 2 / 4
    assert C.share_subnormal(np.ones((3, 3), F32)) == 0.0


def test_route_table_is_well_formed():
    for route, (dtypes, orders, families) in C.ROUTES.items():
        assert dtypes and orders and families, route
        assert set(dtypes) <= {F32, F64} and max(orders) <= 640, route     # no geometry above 640 rows
        assert families in (C.PIVOTED, C.DET_PIVOTED, C.NOPIVOT), route
    assert len(C.all_inversion_cases()) == len(set(C.all_inversion_cases()))


def test_scaling_into_the_subnormal_range_is_not_a_relabelling_of_exponents(oracle):
    """The reason these inputs exist: every step rounds on the subnormal grid, so the oracle's result for gate * 2^-128
    is not 2^128 times its result for gate (an exact scaling of normal numbers would be)."""
    n = 64
    base = C.matrix("gate", n, F32)
    x, st = step_oracle(oracle, base, "gate")
    x_down, st_down = step_oracle(oracle, C.matrix("down", n, F32), "down")
    assert st == st_down == 0
    with np.errstate(over="ignore"):
        relabelled = (x.astype(F64) * 2.0 ** 128).astype(F32)
    assert np.isfinite(relabelled).all() and not np.array_equal(relabelled, x_down)


@pytest.mark.parametrize("dtype,n,family", C.all_inversion_cases(),
                         ids=[f"{np.dtype(d).name}-{n}-{f}" for d, n, f in C.all_inversion_cases()])
def test_every_case_of_the_route_table_meets_the_conditions(oracle, dtype, n, family):
    a = C.matrix(family, n, dtype)
    assert a.dtype == dtype and a.shape == (n, n) and np.isfinite(a).all()
    x, st = step_oracle(oracle, a, family)
    assert st == oracle.STATUS_OK == 0 and np.isfinite(x).all(), (dtype, n, family, st)
    assert C.share_subnormal(subnormal_side(family, a, x)) >= C.MIN_SHARE, (dtype, n, family)


@pytest.mark.parametrize("n", C.ROUTES["blocked32"][1])
@pytest.mark.parametrize("family", C.PIVOTED)
def test_cache_blocked_fp32_oracle_equals_the_in_place_form(oracle, family, n):
    """What the GPU file compares the blocked fp32 path with above 300 rows."""
    a = C.matrix(family, n, F32)
    want, st = step_oracle(oracle, a, family)
    for bw in (64, 128):
        got, info = oracle.matrix_inv_32_blocked_exact(a, n, bw, return_info=True)
        assert info["status"] == st == 0 and canon(got) == canon(want), (family, n, bw)
    aug, info = oracle.matrix_inv_32(a, n, return_info=True)
    assert info["status"] == 0 and canon(aug) == canon(want), (family, n)


@pytest.mark.parametrize("bw", C.F64_BLOCKED_WIDTHS)
@pytest.mark.parametrize("n", C.ROUTES["blocked64"][1])
@pytest.mark.parametrize("family", C.PIVOTED)
def test_fp64_blocked_mirror_takes_these_inputs(oracle, family, n, bw):
    a = C.matrix(family, n, F64)
    x, info = oracle.matrix_inv_64_blocked(a, n, bw, return_info=True)
    assert info["status"] == 0 and x.dtype == F64 and np.isfinite(x).all(), (family, n, bw)
    assert C.share_subnormal(subnormal_side(family, a, x)) >= C.MIN_SHARE, (family, n, bw)


def _check_members(oracle, mats, names, tag):
    """Every member status 0 and finite; per family the conditions on all of its members together."""
    outs = []
    for a, name in zip(mats, names):
        assert np.isfinite(a).all(), (tag, name)
        x, st = step_oracle(oracle, a, name)
        assert st == 0 and np.isfinite(x).all(), (tag, name, a.shape)
        outs.append(x)
    for fam in set(names) - {"gate", "np_plain"}:
        side = np.concatenate([subnormal_side(fam, a, x).reshape(-1) for a, x, nm in zip(mats, outs, names) if nm == fam])
        assert C.share_subnormal(side) >= C.MIN_SHARE, (tag, fam)
    assert len(set(names)) == 3, tag                       # both subnormal families and the ordinary member


@pytest.mark.parametrize("dtype", C.DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("pivoting", [True, False], ids=["pivot", "nopivot"])
def test_mixed_batches_of_the_one_launch_paths(oracle, pivoting, dtype):
    fams = C.batch_families(pivoting)
    for n in C.RESIDENT_ORDERS:
        mats, names = C.mixed_batch(n, C.RESIDENT_BATCH, dtype, fams)
        _check_members(oracle, mats, names, ("resident", n))
    for n in C.WORKGROUP_ORDERS:
        mats, names = C.mixed_batch(n, C.WORKGROUP_BATCH, dtype, fams)
        _check_members(oracle, mats, names, ("workgroup", n))


@pytest.mark.parametrize("dtype", C.DTYPES, ids=["fp32", "fp64"])
def test_ragged_members(oracle, dtype):
    mats, names = C.mixed_members(C.RAGGED_ORDERS * C.RAGGED_COPIES, dtype, C.batch_families(True))
    assert len(mats) == 33 and sorted({m.shape[0] for m in mats}) == sorted(C.RAGGED_ORDERS)
    _check_members(oracle, mats, names, "ragged")
    # every order meets every family: 11 orders and 3 families, member b takes family b % 3
    assert {(m.shape[0], nm) for m, nm in zip(mats, names)} == {(n, f) for n in C.RAGGED_ORDERS
                                                                for f in C.batch_families(True)}


def test_blocked_batch_members(oracle):
    n, fams = C.BLOCKED32_BATCH
    mats, names = C.mixed_members([n] * len(fams), F32, fams)
    assert names == ["down", "up", "gate", "down"] and not np.array_equal(mats[0], mats[3])
    _check_members(oracle, mats, names, "blocked batch")


@pytest.mark.parametrize("dtype", C.DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("pivoting", [True, False], ids=["pivot", "nopivot"])
def test_determinant_mirror_on_subnormal_pivots(oracle, det_dll, pivoting, dtype):
    """The mirror's inverse is the oracle's on these inputs too, the (mantissa, exponent) pair is finite with an
    exponent near E n, and ``det_down`` really hands subnormal pivots to frexp: every pivot of the mirror lies below
    the smallest normal number of its dtype (in fp64: below np.finfo(np.float64).tiny, a subnormal double).  ``down``
    itself cannot do that from n = 16 on, where a pivot of about sqrt(n) 2^-1024 is a normal number again."""
    for n in C.ROUTES["det"][1]:
        for fam in C.ROUTES["det" if pivoting else "det_nopivot"][2]:
            a = C.matrix(fam, n, dtype)
            x, st, piv, _ = mirror(det_dll, a, pivoting)
            ox, ost = step_oracle(oracle, a, fam)
            assert st == ost == 0 and np.array_equal(x, ox), (fam, n)
            _, sts, mant, exp = expected(det_dll, [a], pivoting)
            assert not sts.any() and 0.5 <= abs(mant[0]) < 1.0, (fam, n, mant)
            e = C.exponent(fam, dtype, n)
            assert abs(int(exp[0]) - e * n) <= 6 * n, (fam, n, exp, e * n)      # |log2 pivot - E| < 6: pivots of 2^E
            if fam == "det_down":
                assert C.share_subnormal(piv) == 1.0, (n, dtype)                 # every pivot, in fp32 and in fp64


@pytest.mark.parametrize("dtype", C.DTYPES, ids=["fp32", "fp64"])
def test_solve_mirror_on_subnormal_systems(solve_dll, dtype):
    for n, k in sorted(set(C.solve_shapes() + [(n, k) for k, orders in C.SOLVE_RAGGED.items() for n in orders])):
        for fam in C.PIVOTED:
            a, b = C.matrix(fam, n, dtype), C.solve_rhs(fam, n, k, dtype)
            assert b.dtype == dtype and np.isfinite(a).all() and np.isfinite(b).all()
            x, st = mirror_solve(solve_dll, a, b)
            assert st == 0 and np.isfinite(x).all(), (fam, n, k)
            if fam == "down":
                assert C.share_subnormal(a) >= C.MIN_SHARE and C.share_subnormal(b) >= 0.99, (n, k)
                assert C.share_subnormal(x) == 0.0, (n, k)                       # X ordinary
            else:
                assert C.share_subnormal(b) == 0.0 and C.share_subnormal(x) >= C.MIN_SHARE_SOLVE_UP, (n, k)


def test_output_overflow_is_status_0_in_both_oracle_forms(oracle):
    """Every pivot finite, so status 0; the inverse overflows: wholly non-finite at n = 3 and 8, 63 finite entries of
    256 at n = 16.  The status looks at pivots and input entries only."""
    finite = {3: 0, 8: 0, 16: 63}
    assert tuple(finite) == C.OVERFLOW_OUT_ORDERS
    for n in C.OVERFLOW_OUT_ORDERS:
        a = C.overflow_out(n)
        assert a.dtype == F32 and np.isfinite(a).all() and C.share_subnormal(a) >= C.MIN_SHARE
        x, info = oracle.matrix_inv_32_inplace(a, n, return_info=True)
        aug, info_aug = oracle.matrix_inv_32(a, n, return_info=True)
        assert info["status"] == info_aug["status"] == 0, n
        assert int(np.isfinite(x).sum()) == finite[n], n
        assert C.same_with_nonfinite(aug, x) and C.same_with_nonfinite(x, x), n
    bad = np.array([np.inf, 1.0], F32)
    assert not C.same_with_nonfinite(bad, -bad) and not C.same_with_nonfinite(bad, np.array([np.nan, 1.0], F32))
    assert C.same_with_nonfinite(np.array([np.nan, -0.0], F32), np.array([-np.nan, 0.0], F32))


def test_residuals_of_the_verifier_cases_are_finite(oracle):
    n = C.ROUTES["residual"][1][0]
    for fam in C.PIVOTED:
        a = C.matrix(fam, n, F32)
        x, st = step_oracle(oracle, a, fam)
        assert st == 0
        r, rl = oracle.residual_inf(a, x, n), oracle.residual_inf_left(a, x, n)
        assert np.isfinite(r) and np.isfinite(rl) and 0 < r < 1e-2 and 0 < rl < 1e-2, (fam, r, rl)
