"""CPU-only proof that the inputs of tests/nopivot_cases.py are what they claim to be, and that the oracle's no-pivot
restatement -- the reference of tests/test_gpu_nopivot.py -- is right where these inputs take it: off the diagonally
dominant matrices on which tests/test_oracle.py pins it.  A precondition of the GPU tests, not a measurement."""
import numpy as np
import pytest

import fp64_cases
import nopivot_cases as C
from conftest import forward_tolerance

DTYPES = [np.float32, np.float64]
IDS = ["fp32", "fp64"]
needs_extended = pytest.mark.skipif(not fp64_cases.longdouble_is_extended(),
                                    reason="np.longdouble is not an extended format")


def no_pivot(oracle, a):
    n = a.shape[0]
    x, info = oracle.matrix_inversion_no_pivots(a, n, return_info=True)
    assert x.dtype == a.dtype
    return x.reshape(n, n), int(info["status"])


def check_claims(name, n, dtype, a):
    """The documented properties of family ``name`` at order n: the test fails if a generator stops having them."""
    assert a.dtype == dtype and a.shape == (n, n) and np.isfinite(a).all()
    share = C.dominant_share(a)
    zeros = C.exact_zeros(a)
    outside = C.diagonal_outside_division_range(a)
    negative = C.negative_diagonal(a)
    tag = (name, n, dtype.__name__, share, zeros, outside, negative)
    if name in ("spd", "spd_signed"):
        assert np.array_equal(np.abs(a), np.abs(a.T)), tag
        assert share < 1.0 if n < 9 else share == 0.0, tag                   # from n = 9 on no row is dominant
        assert zeros == 0 and outside == 0, tag
        if name == "spd":
            assert negative == 0, tag
        else:
            neg = C.negated_rows(n, C.seed_of(n))
            assert negative == len(neg) and (np.diag(a)[neg] < 0).all(), tag   # exactly the negated rows:
            assert n < 64 or 0.3 <= negative / n <= 0.7, tag                   # about half of the pivots
    elif name == "spd_scaled":
        assert np.array_equal(a, a.T) and zeros == 0 and negative == 0, tag
        assert share < (0.1 if n >= 64 else 0.5), tag
        # |e| >= 24 puts 0.38 * 2^(2 e) outside: 14 of 61 exponents in fp32, about 452 of 501 in fp64 -- between a fifth
        # and nine tenths of the diagonal; a wider window where 64 ... 257 draws scatter more
        if n >= 500:
            lo, hi = (0.18, 0.30) if dtype == np.float32 else (0.85, 0.95)
            assert lo <= outside / n <= hi, tag
        elif n >= 64:
            lo, hi = (0.10, 0.40) if dtype == np.float32 else (0.75, 1.0)
            assert lo <= outside / n <= hi, tag
        if n >= 8:
            assert outside >= 1, tag
    elif name == "sparse_spd":
        assert np.array_equal(a, a.T) and outside == 0 and negative == 0, tag
        assert zeros >= 0.6 * n * n, tag                                     # exact-zero multipliers at every step
        if n == 1000:
            assert 0.62 <= zeros / n ** 2 <= 0.72, tag                       # "about two thirds"
        if n >= 512:
            assert share <= 0.01, tag                                        # not dominant (a stray row at most)
        assert (a != 0).sum(axis=1).min() >= 1, tag
    else:
        assert name == "tridiagonal"
        assert C.weakly_dominant_share(a) == 1.0, tag                        # weakly dominant only:
        assert share == min(2, n) / n, tag                                   # strictly in the first and last row
        assert zeros == n * n - (3 * n - 2) and outside == 0 and negative == 0, tag


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", C.ALL_ORDERS)
def test_families_are_what_they_claim_and_the_oracle_inverts_them(oracle, n, dtype):
    got = {}
    for name in C.FAMILIES:
        a = C.family(name, n, dtype)
        check_claims(name, n, dtype, a)
        x, st = no_pivot(oracle, a)
        assert st == C.STATUS_OK == oracle.STATUS_OK, (name, n)
        assert np.isfinite(x).all(), (name, n)
        got[name] = x
    # the two identities that hold bit for bit: scaling by powers of two and negating rows are exact
    seed = C.seed_of(n)
    assert np.array_equal(C.unscale(got["spd_scaled"], n, seed, dtype), got["spd"]), n
    want = got["spd"].copy()
    want[:, C.negated_rows(n, seed)] *= -1
    assert np.array_equal(got["spd_signed"], want), n


def test_the_lookahead_case(oracle):
    n = C.LOOKAHEAD_ORDER
    a = C.family("spd_scaled", n, np.float32)
    check_claims("spd_scaled", n, np.float32, a)
    x, st = no_pivot(oracle, a)
    assert st == C.STATUS_OK and np.isfinite(x).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_side_by_side_batches(oracle, dtype):
    """The batches of the one-launch paths: every member regular, both signs of determinant among the signed ones."""
    parities = set()
    for n in C.RESIDENT_ORDERS + C.WORKGROUP_ORDERS:
        mats, names, seeds = C.side_by_side(n, dtype)
        assert len(mats) == 15 and names[:5] == list(C.FAMILIES)
        for b, a in enumerate(mats):
            x, st = no_pivot(oracle, a)
            assert st == C.STATUS_OK and np.isfinite(x).all(), (n, b, names[b])
        assert len({mats[b].tobytes() for b in range(15) if names[b] == "spd"}) == 3, n   # the copies differ
        parities |= {len(C.negated_rows(n, seeds[b])) % 2 for b in range(15) if names[b] == "spd_signed"}
    assert parities == {0, 1}


def test_scaled_multipliers_are_far_from_one():
    """What spd_scaled is for: multipliers of the elimination of about 2^37 and above in fp32 (no dominant input has
    one above 1), next to tiny ones."""
    n = 513
    a = C.family("spd_scaled", n, np.float32).astype(np.float64)
    biggest, smallest = 0.0, np.inf
    m = a.copy()
    for r in range(n - 1):                       # plain Gaussian elimination below the diagonal is enough to see them
        f = m[r + 1:, r] / m[r, r]
        biggest = max(biggest, np.abs(f).max())
        smallest = min(smallest, np.abs(f[f != 0]).min())
        m[r + 1:, r + 1:] -= f[:, None] * m[r, r + 1:][None, :]
    assert biggest >= 2.0 ** 37 and smallest <= 2.0 ** -37, (np.log2(biggest), np.log2(smallest))


@pytest.mark.parametrize("path,dtype,n,bw,steps", C.ZERO_PIVOTS,
                         ids=[f"{p}-{np.dtype(d).name}-{n}-{bw}" for p, d, n, bw, _ in C.ZERO_PIVOTS])
def test_every_zero_pivot_position_is_status_2(oracle, path, dtype, n, bw, steps):
    base = C.family("spd", n, dtype)
    for k in steps:
        a = C.zero_pivot_at(base, k)
        assert a[k, k] == 0 and not a[k].any() and not a[:, k].any() and np.isfinite(a).all()
        assert no_pivot(oracle, a)[1] == C.STATUS_SINGULAR == oracle.STATUS_SINGULAR, (path, n, k)
        if k:    # the steps before k are those of a regular matrix: the leading block is SPD
            lead = C.zero_pivot_at(base, k)[:k, :k]
            assert no_pivot(oracle, lead)[1] == C.STATUS_OK, (path, n, k)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_status_batch(oracle, dtype):
    mats, want = C.status_batch(dtype)
    assert want == [0, 2, 0, 0]
    for b, a in enumerate(mats):
        x, st = no_pivot(oracle, a)
        assert st == want[b], b
        if st == C.STATUS_OK:
            assert np.isfinite(x).all(), b
    k = C.BATCH_CANCEL_STEP
    assert np.array_equal(mats[3][k], mats[3][k + 1])
    # near_cancellation: huge next to the regular member's inverse (7.3), and finite
    big = np.abs(no_pivot(oracle, mats[3])[0]).max()
    assert big > 1e6 * np.abs(no_pivot(oracle, mats[0])[0]).max()


# ---- the oracle's no-pivot restatement against an elimination that does not go through the oracle ---------------------
def plain_elimination(a, wide):
    """In-place Gauss-Jordan without pivoting in the wider type ``wide``, written in numpy."""
    m = np.array(a, dtype=wide)
    n = m.shape[0]
    for r in range(n):
        piv = m[r, r]
        row = m[r] / piv
        row[r] = 1 / piv
        col = m[:, r].copy()
        col[r] = 0
        m[:, r] = 0
        m -= col[:, None] * row[None, :]
        m[r] = row
    return m


INDEPENDENT_ORDERS = (5, 64, 257, 513)


@pytest.mark.parametrize("dtype", [np.float32, pytest.param(np.float64, marks=needs_extended)], ids=IDS)
@pytest.mark.parametrize("name", ["spd", "sparse_spd", "tridiagonal"])
def test_oracle_no_pivot_restatement_against_a_plain_elimination(oracle, name, dtype):
    """float64 for fp32 inputs, np.longdouble for fp64 inputs.  The bound is the project's own forward bound, factor 2:
    max|X - Xref| / max|Xref| <= 2 kappa_inf(A) u with u = 2^-24 (conftest.forward_tolerance) or 2^-53
    (fp64_cases.forward_bound).  The oracle stays inside it on every case here: measured at most 0.375 kappa_inf u
    (sparse_spd at n = 5 in fp32, a diagonal matrix there; 0.06 kappa_inf u at most from n = 64 on), so the project's
    bound is taken as it is."""
    for n in INDEPENDENT_ORDERS:
        a = C.family(name, n, dtype)
        x, st = no_pivot(oracle, a)
        assert st == C.STATUS_OK
        if dtype == np.float32:
            ref = plain_elimination(a, np.float64)
            bound = forward_tolerance(a, 2.0)
        else:
            ref = plain_elimination(a, np.longdouble)
            bound = fp64_cases.forward_bound(a, ref, 2.0)
        # the wide elimination really inverts: its own residual is far below what the oracle is held to
        assert fp64_cases.residual_inf_longdouble(a, ref) <= bound / 16, (name, n)
        err = fp64_cases.forward_error(x, ref)
        print(f"{name} n={n} {np.dtype(dtype).name}: error {err:.3e}, bound {bound:.3e}, ratio {err / bound:.4f}")
        assert err <= bound, (name, n, err, bound)
