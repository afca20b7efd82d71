"""GPU tests of the residual verifier (``residual_tile_kernel`` / ``residual_finalize_kernel``) at its tile edges, through
``Inverter.residual`` and ``matrix_multiply`` (run with ``-m gpu`` on an MI355X).  Every accuracy claim of this project
that is not a bit-for-bit comparison rests on this kernel, so it is judged by answers no product routine computed:
the cases of tests/residual_cases.py, proved on the CPU oracle by tests/test_residual_cases.py.

Integer operands and planted errors are compared with ``==``.  The only tolerances are those of residual_cases:
``frobenius_tolerance_exact`` (two square roots and a subtraction) and ``float_tolerances`` (a-priori bounds from the
operands); none comes from the kernel's output.
"""
import numpy as np
import pytest

from residual_cases import (FLOAT_ORDERS, ORDERS, all_positions, edge_positions, expected_exact, float_inputs,
                            float_tolerances, frobenius_tolerance_exact, integer_batch, integer_pair, planted, planted_batch)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_matrix_inversion_amd as g  # noqa: E402

FULL_ORDERS = [65, 68]   # every position: one order of the scalar-load branch, one of the 16-byte-load branch
DELTAS = pytest.mark.parametrize("delta", [1.0, 2.0 ** -20], ids=["1", "2^-20"])


@pytest.fixture(scope="module")
def inv():
    h = g.Inverter(algo="sweep")
    yield h
    h.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def res(inv, a, x):
    """The (B, 3) float64 result of Inverter.residual on numpy operands."""
    return inv.residual(dev(a), dev(x)).cpu().numpy()


def check_exact(got, a, x, tag):
    """One row of the verifier against the int64 answer: the norms with ==, the metric within two square roots."""
    want = expected_exact(a, x)
    assert got[0] == want[0] and got[1] == want[1], (tag, got, want)
    assert abs(got[2] - want[2]) <= frobenius_tolerance_exact(a, x), (tag, got[2], want[2])


# ---- 1. exact integers, every order ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ORDERS)
def test_integer_pair_every_order(inv, n):
    a, x = integer_pair(n, 7)
    fwd = res(inv, a, x)
    assert fwd.shape == (1, 3) and fwd.dtype == np.float64
    check_exact(fwd[0], a, x, n)
    # swapped operands: the two norms swap (a mixed-up `which` would not), the metric is that of X A
    back = res(inv, x, a)[0]
    assert back[0] == fwd[0][1] and back[1] == fwd[0][0], (n, fwd, back)
    check_exact(back, x, a, (n, "swapped"))


# ---- 2. one wrong entry raises the residual by the right amount -----------------------------------------------------
def check_planted(inv, n, positions, delta):
    a, x, want = planted_batch(n, 11, positions, delta)
    got = res(inv, a, x)
    bad = np.nonzero((got[:, 0] != want[:, 0]) | (got[:, 1] != want[:, 1]))[0]
    assert bad.size == 0, (n, delta, [(positions[b], got[b, :2].tolist(), want[b].tolist()) for b in bad[:8]])


@DELTAS
@pytest.mark.parametrize("n", FULL_ORDERS)
def test_planted_error_every_position(inv, n, delta):
    """One batch, one member per position of the wrong entry: 4225 and 4624 members in one call."""
    positions = all_positions(n)
    assert len(positions) == n * n
    check_planted(inv, n, positions, delta)


@pytest.mark.parametrize("n", [n for n in ORDERS if n not in FULL_ORDERS])
def test_planted_error_at_the_tile_edges(inv, n):
    """The corners and both sides of every 16 / 32 / 64 boundary that exists at this order, rows and columns."""
    for delta in (1.0, 2.0 ** -20):
        check_planted(inv, n, edge_positions(n), delta)


def test_exact_inverse_has_zero_residual(inv):
    for n in (5, 65, 68):
        a, x, _ = planted(n, 11, 0, 0, 0.0)
        assert res(inv, a, x)[0].tolist() == [0.0, 0.0, 0.0]


# ---- 3. float operands against the oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", FLOAT_ORDERS)
def test_float_operands_against_the_oracle(oracle, inv, n):
    for name, a in float_inputs(n).items():
        ta = dev(a)
        tx, st = inv.inv(ta)
        got = inv.residual(ta, tx).cpu().numpy()[0]
        x = tx.cpu().numpy()
        assert st.cpu().numpy().tolist() == [0]
        want = (oracle.residual_inf(a, x, n), oracle.residual_inf_left(a, x, n), oracle.frobenius_metric(a, x, n))
        tol_r, tol_f = float_tolerances(a, x)
        tol_l, _ = float_tolerances(x, a)
        print(f"n={n} {name}: got {got.tolist()} oracle {want} bounds {(tol_r, tol_l, tol_f)}")
        assert abs(got[0] - want[0]) <= tol_r, (n, name, got[0], want[0], tol_r)
        assert abs(got[1] - want[1]) <= tol_l, (n, name, got[1], want[1], tol_l)
        assert abs(got[2] - want[2]) <= tol_f, (n, name, got[2], want[2], tol_f)


# ---- 4. batches -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 64, 65])
def test_batch_rows_equal_the_single_calls(inv, n):
    a, x = integer_batch(n, 7, 3)
    got = res(inv, a, x)
    assert got.shape == (7, 3)
    for b in range(7):
        check_exact(got[b], a[b], x[b], (n, b))
        assert got[b].tolist() == res(inv, a[b], x[b])[0].tolist(), (n, b)


def test_workspace_of_a_larger_order_does_not_leak_into_the_next_call():
    h = g.Inverter(algo="sweep")
    try:
        big, small = integer_pair(130, 5), integer_pair(5, 5)
        first = res(h, *big)[0]
        check_exact(first, *big, "130")
        check_exact(res(h, *small)[0], *small, "5 after 130")
        assert res(h, *big)[0].tolist() == first.tolist()
    finally:
        h.close()


def test_on_a_side_stream_right_after_an_inversion(inv):
    """The inversion leaves its own data in the workspace the row sums go to; the verifier is queued behind it."""
    n = 130
    a, x = integer_pair(n, 9)
    ta, tx = dev(a), dev(x)
    tg = dev(float_inputs(n)["gate"])
    want = inv.residual(ta, tx).cpu().numpy()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        xg, st = inv.inv(tg)
        r = inv.residual(ta, tx)
        rg = inv.residual(tg, xg)
    s.synchronize()
    check_exact(r.cpu().numpy()[0], a, x, "side stream")
    assert r.cpu().numpy().tolist() == want.tolist()
    assert int(st.item()) == 0 and 0.0 < float(rg[0, 0]) < 1e-3
    torch.cuda.synchronize()


# ---- 5. more members than one grid takes ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 4])
def test_70000_members(inv, n):
    B = 70_000
    a, x = integer_batch(n, B, 13)
    special = [0, 65_534, 65_535, 65_536, 69_999]
    for k, b in enumerate(special):   # a wrong entry of its own size in the members around the grid's z limit
        a[b], x[b], _ = planted(n, 13, k % n, (k + 1) % n, float(k + 1))
    want = expected_exact(a, x)       # one vectorised int64 einsum
    assert want.shape == (B, 3)
    assert want[special, 0].tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]
    got = res(inv, a, x)
    assert got.shape == (B, 3)
    bad = np.nonzero((got[:, 0] != want[:, 0]) | (got[:, 1] != want[:, 1]))[0]
    assert bad.size == 0, (n, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    assert (np.abs(got[:, 2] - want[:, 2]) <= frobenius_tolerance_exact(a, x)).all()


# ---- 6. non-finite operands -----------------------------------------------------------------------------------------
NONFINITE_ORDERS = [5, 65, 68, 130]


def _positions(n):
    # first row, last row, and the last entry: inside the last (partial) tile
    return [(0, n // 2), (n - 1, 0), (n - 1, n - 1)]


@pytest.mark.parametrize("n", NONFINITE_ORDERS)
def test_nan_entry_gives_nan_in_all_three_outputs(oracle, inv, n):
    a, x = integer_pair(n, 17)
    for i, j in _positions(n):
        for in_x in (True, False):
            a1, x1 = a.copy(), x.copy()
            (x1 if in_x else a1)[i, j] = np.nan
            got = res(inv, a1, x1)[0]
            assert np.isnan(got).all(), (n, i, j, in_x, got)
            want = (oracle.residual_inf(a1, x1, n), oracle.residual_inf_left(a1, x1, n), oracle.frobenius_metric(a1, x1, n))
            assert np.isnan(want).all()


@pytest.mark.parametrize("value", [np.inf, -np.inf], ids=["+inf", "-inf"])
@pytest.mark.parametrize("n", NONFINITE_ORDERS)
def test_infinite_entry_gives_what_the_oracle_gives(oracle, inv, n, value):
    a, x = integer_pair(n, 19)
    nz = np.where(a == 0, np.float32(1), a)   # no zero entry: an infinity stays an infinity
    for i, j in _positions(n):
        x1 = x.copy()
        x1[i, j] = value
        for a1, literal in ((nz, [np.inf, np.inf, -np.inf]), (a, None)):
            if literal is None:
                a1 = a.copy()
                a1[0, i] = 0          # 0 * inf in column j of A X: NaN there
            got = res(inv, a1, x1)[0]
            want = np.array([oracle.residual_inf(a1, x1, n), oracle.residual_inf_left(a1, x1, n),
                             oracle.frobenius_metric(a1, x1, n)])
            assert np.array_equal(got, want, equal_nan=True), (n, i, j, value, got, want)
            if literal is not None:
                assert got.tolist() == literal
            else:
                assert np.isnan(got[0]) and np.isnan(got[2])


@pytest.mark.parametrize("n", NONFINITE_ORDERS)
def test_nan_member_does_not_touch_its_neighbours(inv, n):
    a, x = integer_batch(n, 3, 23)
    x[1, n - 1, n - 1] = np.nan
    got = res(inv, a, x)
    assert np.isnan(got[1]).all()
    for b in (0, 2):
        check_exact(got[b], a[b], x[b], (n, b))
        assert got[b].tolist() == res(inv, a[b], x[b])[0].tolist()


# ---- 7. matrix_multiply: the double instance of the tile kernel -----------------------------------------------------
@pytest.mark.parametrize("n", ORDERS)
def test_matrix_multiply_integer_pair(n):
    a, x = integer_pair(n, 7)
    got = g.matrix_multiply(a.astype(np.float64), x.astype(np.float64))
    want = expected_exact(a, x)[2]
    assert abs(got - want) <= frobenius_tolerance_exact(a, x), (n, got, want)


@pytest.mark.parametrize("n", [5, 65, 100, 130])
def test_matrix_multiply_float64_against_a_longdouble_product(n):
    rng = np.random.default_rng([29, n])
    a, b = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    c = a.astype(np.longdouble) @ b.astype(np.longdouble)
    want = float(np.sqrt(np.longdouble(n)) - np.sqrt((c * c).sum()))
    got = g.matrix_multiply(a, b)
    tol = float_tolerances(a, b)[1]
    print(f"n={n}: got {got!r} longdouble {want!r} bound {tol!r}")
    assert abs(got - want) <= tol, (n, got, want, tol)


# ---- 8. the host side refuses what the kernel cannot take -----------------------------------------------------------
def test_residual_refuses_bad_operands(inv):
    a, x = (dev(m) for m in integer_pair(8, 1))
    a3, x3 = (dev(m) for m in integer_batch(8, 3, 1))
    assert inv.residual(a, x).shape == (1, 3) and inv.residual(a3, x3).shape == (3, 3)
    bad = {
        "float64 a": (a.double(), x), "float64 x": (a, x.double()), "both float64": (a.double(), x.double()),
        "int32": (a.int(), x.int()),
        "x with fewer members": (a3, x3[:2]), "x with more members": (a3[:2], x3), "x single, a batch": (a3, x),
        "another order": (a, x[:7, :7]), "another order in a batch": (a3, x3[:, :7, :7]),
        "not square": (a[:, :7], x[:, :7]), "one-dimensional": (a.reshape(-1), x.reshape(-1)),
        "empty batch": (a3[:0], x3[:0]),
        "CPU a": (a.cpu(), x), "CPU x": (a, x.cpu()), "both on the CPU": (a.cpu(), x.cpu()),
    }
    for what, (l, r) in bad.items():
        with pytest.raises(ValueError):
            inv.residual(l, r)
            pytest.fail(f"accepted: {what}")
    # and the handle is as good as before
    assert inv.residual(a, x).cpu().numpy()[0, :2].tolist() == list(expected_exact(a.cpu().numpy(), x.cpu().numpy())[:2])


def test_residual_refuses_a_tensor_on_another_device(inv):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    other = torch.device("cuda", (inv.device.index + 1) % torch.cuda.device_count())
    a, x = (dev(m) for m in integer_pair(8, 1))
    for l, r in ((a.to(other), x), (a, x.to(other)), (a.to(other), x.to(other))):
        with pytest.raises(ValueError):
            inv.residual(l, r)
