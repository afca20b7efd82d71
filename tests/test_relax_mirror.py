"""CPU tests of the relaxation mirror (tests/relax_mirror.c through tests/relax_cases.py), the expectation every GPU test
of tests/test_gpu_relax.py compares bytes with: the residual rule of include/mat_inv_32_relax.h against an exact
residual within a derived bound, exactly on integer inputs, under permutations of a row's entries, and the sweep built
on it converging at the rate diagonal dominance promises.  No library call, no GPU."""
import math

import numpy as np
import pytest

import relax_cases as rc
from apply_cases import assert_same_bits, build_apply_mirror

DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])


@pytest.fixture(scope="module")
def dll(tmp_path_factory):
    return rc.build_relax_mirror(tmp_path_factory.mktemp("relax_mirror"))


@pytest.fixture(scope="module")
def adll(tmp_path_factory):
    return build_apply_mirror(tmp_path_factory.mktemp("apply_mirror"))


def unit(dtype):
    return 2.0 ** -24 if dtype == np.float32 else 2.0 ** -53


@DTYPES
def test_residual_within_the_derived_bound(dll, dtype):
    """Every entry of a row passes through at most ceil(c / 8) fused multiply-adds of its partial sum, three butterfly
    additions and the subtraction from b, each one rounding: k = ceil(c / 8) + 4 roundings, so the standard bound is
    |r - r_exact| <= gamma_k (sum |a||x| + |b|), gamma_k = k u / (1 - k u).  The reference is the residual in float64
    for the float mirror (products of two floats are exact there, ``math.fsum`` adds them exactly) and in longdouble
    for the double mirror.  Rows of 0 ... 40 entries and one of 700."""
    n = 800
    lengths = [i % 41 for i in range(n)]
    lengths[5] = 700
    csr = rc.random_rows(n, lengths, 3, dtype)
    rng = np.random.default_rng(4)
    x, b = rng.uniform(-1, 1, n).astype(dtype), rng.uniform(-1, 1, n).astype(dtype)
    r = rc.mirror_residual(dll, csr, x, b, np.arange(n))
    crow, col, val = csr
    wide = np.float64 if dtype == np.float32 else np.longdouble
    u, worst = unit(dtype), 0.0
    for g in range(n):
        a, xs = val[crow[g]:crow[g + 1]].astype(wide), x[col[crow[g]:crow[g + 1]]].astype(wide)
        terms = a * xs
        exact = wide(b[g]) - (wide(math.fsum(terms)) if wide is np.float64 else terms.sum(dtype=wide))
        k = -(-lengths[g] // 8) + 4
        bound = k * u / (1 - k * u) * float(np.abs(terms).sum() + abs(wide(b[g])))
        err = abs(float(wide(r[g]) - exact))
        worst = max(worst, err / bound if bound else 0.0)
        assert err <= bound, (g, lengths[g], err, bound)
    print(f"\n largest error / bound over {n} rows: {worst:.3f}")
    assert_same_bits(r[[0, 41]], b[[0, 41]], "an empty row: r = b - (+0)")


@DTYPES
def test_exact_on_integer_inputs(dll, dtype):
    """Small integers: every product and every sum is exact, so r is the integer residual."""
    n = 720
    lengths = [i % 23 for i in range(n)]
    lengths[7] = 700
    crow, col, _ = rc.random_rows(n, lengths, 8, dtype)
    rng = np.random.default_rng(9)
    val = rng.integers(-8, 9, col.size)
    x, b = rng.integers(-8, 9, n), rng.integers(-100, 101, n)
    want = b - np.array([int((val[crow[g]:crow[g + 1]] * x[col[crow[g]:crow[g + 1]]]).sum()) for g in range(n)])
    assert np.abs(want).max() < 2 ** 24
    got = rc.mirror_residual(dll, (crow, col, val.astype(dtype)), x.astype(dtype), b.astype(dtype), np.arange(n))
    assert_same_bits(got, want.astype(dtype), "integers")


def _one_row(values, dtype, n=32):
    """A matrix whose row 0 holds `values` in this stored order, entry e at column e (x = 1 everywhere)."""
    cols = [np.arange(len(values))] + [np.zeros(0, np.int64)] * (n - 1)
    vals = [np.asarray(values, dtype)] + [np.zeros(0, dtype)] * (n - 1)
    return rc.csr_of_rows(cols, vals, dtype)


@DTYPES
def test_stored_order_enters_the_way_the_rule_says(dll, dtype):
    """big = 1 / u is where the spacing becomes 2: big + 1 rounds back to big (a tie, to even).  With big, 1, -big all in
    partial sum 0 (entries 0, 8, 16) the one is lost and the sum is 0; with them in the partial sums 0, 1, 2 (entries 0,
    1, 2) the butterfly adds p_0 + p_2 = 0 first and the sum is 1.  A permutation of the entries that maps partial sum
    s to s xor 1, 2 or 4 changes no bit (the butterfly's additions are commutative); one that rotates s does."""
    big = 1.0 / unit(dtype)             # 2^24 / 2^53
    x, b = np.ones(32, dtype), np.zeros(32, dtype)
    same_class = np.zeros(17)
    same_class[[0, 8, 16]] = big, 1.0, -big
    r = rc.mirror_residual(dll, _one_row(same_class, dtype), x, b, [0])
    assert r[0] == 0.0
    r = rc.mirror_residual(dll, _one_row([big, 1.0, -big], dtype), x, b, [0])
    assert r[0] == -1.0
    # p_0 + p_4 first: big and -big four entries apart cancel before the one arrives
    r = rc.mirror_residual(dll, _one_row([big, 1.0, 0, 0, -big], dtype), x, b, [0])
    assert r[0] == -1.0
    # ... and one entry apart they meet only at the last level, after big + 1 has lost the one in t_0: q_0 = big, q_1 =
    # -big, q_2 = 1; t_0 = q_0 + q_2 = big, t_1 = -big; sum = 0
    r = rc.mirror_residual(dll, _one_row([big, -big, 1.0], dtype), x, b, [0])
    assert r[0] == 0.0
    rng = np.random.default_rng(10)
    values = (rng.uniform(0.25, 1.0, 40) * rng.choice([-1.0, 1.0], 40) * 2.0 ** rng.integers(-6, 7, 40)).astype(dtype)
    base = rc.mirror_residual(dll, _one_row(values, dtype, 64), np.ones(64, dtype), np.zeros(64, dtype), [0])
    e = np.arange(40)
    for bit in (1, 2, 4):
        moved = np.empty_like(values)
        moved[e ^ bit] = values           # entry e goes to e xor bit: partial sum s becomes s xor bit, same order inside
        got = rc.mirror_residual(dll, _one_row(moved, dtype, 64), np.ones(64, dtype), np.zeros(64, dtype), [0])
        assert_same_bits(got, base, ("xor", bit))
    changed = 0
    for seed in range(20):
        v = (np.random.default_rng(seed).uniform(0.25, 1.0, 40) * 2.0 ** np.random.default_rng(seed).integers(-6, 7, 40))
        v = v.astype(dtype)
        one = rc.mirror_residual(dll, _one_row(v, dtype, 64), np.ones(64, dtype), np.zeros(64, dtype), [0])
        two = rc.mirror_residual(dll, _one_row(np.roll(v, 1), dtype, 64), np.ones(64, dtype), np.zeros(64, dtype), [0])
        changed += one[0] != two[0]
    assert changed > 0


@DTYPES
def test_mirror_sweep_converges_at_the_rate_of_diagonal_dominance(dll, adll, dtype):
    """The matrix of ``relax_cases.jacobi_matrix``: N = 1177, dense diagonal blocks of orders 1 ... 40, 64, 65, 100, 128,
    four entries per row outside the block, a_ii = 4 sum_{j != i} |a_ij|.  With M = blockdiag(A) and s_in / s_off the
    off-diagonal row sums inside / outside the block, ||I - M^-1 A||_inf = ||M^-1 (A - M)||_inf <= max_i s_off / (a_ii -
    s_in) = max_i s_off / (3 s_in + 4 s_off) <= 1/4, asserted in float64 at 1/3.  Hence ||x_k - x*|| <= (1/3)^k ||x*||
    from x_0 = 0 in exact arithmetic (norms are infinity norms, x* = A^-1 b in float64).

    The rounding allowance 64 u ||x*||.  Rows hold at most c = 128 + 4 entries, so a residual has k_r = ceil(132 / 8) + 4
    = 21 roundings; the product of a block of order n is a chain of n <= 128 roundings; the last fma is one.  Write
    e_k = x_k - x*.  Per row |b_i| and sum |a||x*| are at most (5/4) a_ii ||x*||, and ||M^-1 v|| <= max_i |v_i| / (a_ii -
    s_in) <= (4/3) max_i |v_i| / a_ii; the same holds for |M^-1| |v|.  First order in u, per sweep:
      * residual: (4/3) (5/4) gamma_21 (||x_k|| + ||x*||) <= (5/3) 21 u (7/3) ||x*|| = 82 u ||x*|| in the WORST case -- but in
        sweep 1 x_0 = 0 and r = b exactly;
      * product: gamma_n (|X| |r|) <= 128 u (5/3) ||e_k||, i.e. 213 u ||x*|| in sweep 1 and a third of that per later one;
      * the members are the float64 inverses rounded to the working type: a relative change u of X, which moves the
        iteration matrix by at most (5/3) u and leaves the fixed point x* where it is;
      * last fma: u ||x_k+1|| (exact in sweep 1, where x_0 = 0).
    Errors of earlier sweeps contract with the iteration, so the total is at most 3/2 of the largest.  The worst-case
    constants above EXCEED 64: no first-order worst-case analysis of a 128-term chain can promise less than 128 u.  The
    allowance is that of rounding errors that do not all point the same way, the model behind the bound gamma~_n =
    lambda sqrt(n) u (Higham and Mary, 2019): with lambda = 3, product sqrt(128) 3 (5/3) u = 57 u ||x*|| in sweep 1,
    residual sqrt(21) 3 (5/3) (7/3) u = 54 u ||x*|| later, both under 64 u.  The measured figures are printed, the floor
    of the iteration among them."""
    csr, orders, first = rc.jacobi_matrix(dtype)
    a = rc.dense_of(csr)
    n = a.shape[0]
    assert n == 1177 and sorted(orders) == sorted(list(range(1, 41)) + [64, 65, 100, 128])
    m = np.zeros_like(a)
    for f, k in zip(first, orders):
        m[f:f + k, f:f + k] = a[f:f + k, f:f + k]
    rate = np.abs(np.eye(n) - np.linalg.solve(m, a)).sum(axis=1).max()
    print(f"\n ||I - M^-1 A||_inf = {rate:.4f}")
    assert rate <= 1 / 3
    xstar = np.random.default_rng(6).uniform(-1, 1, n).astype(dtype).astype(np.float64)
    b = (a @ xstar).astype(dtype)
    xstar = np.linalg.solve(a, b.astype(np.float64))
    wide = rc.block_inverses(csr, orders, first, dtype)
    u, scale = unit(dtype), np.abs(xstar).max()
    x = np.zeros(n, dtype)
    for k in range(1, 5):
        x = rc.mirror_sweep(dll, adll, csr, first, wide, x, b)
        err = np.abs(x.astype(np.float64) - xstar).max()
        bound = ((1 / 3) ** k + 64 * u) * scale
        print(f" sweep {k}: ||x_k - x*|| / ||x*|| = {err / scale:.3e}  (bound {bound / scale:.3e}, in u: {err / scale / u:.1f})")
        assert err <= bound, (k, err, bound)
    # the floor the iteration settles at is the rounding term alone: printed beside the allowance, not asserted
    floor = rc.mirror_sweep(dll, adll, csr, first, wide, x, b, sweeps=30 if dtype == np.float64 else 12)
    print(f" floor: ||x - x*|| / ||x*|| = {np.abs(floor.astype(np.float64) - xstar).max() / scale / u:.2f} u  (allowance 64 u)")
    # k sweeps in one call of the mirror are the k calls
    assert_same_bits(rc.mirror_sweep(dll, adll, csr, first, wide, np.zeros(n, dtype), b, sweeps=4), x, "sweeps")
