"""The fp64 no-pivot variant (matrix_inversion_no_pivots of the reference, headers.h:11) on its blocked path
(mi32_nopivot64.hip): AUTO from N = 512 on, explicit ``algo="blocked"`` at any order.  Every result is compared bit for
bit (``np.array_equal``) with the oracle's no-pivot restatement, which is what the sweep kernels return.  Every valid
input here is strictly diagonally dominant with a positive diagonal; tests/test_gpu_nopivot.py runs the same path on
inputs that are not (tests/nopivot_cases.py)."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_matrix_inversion_amd as g  # noqa: E402


def dominant(n, seed):
    """U(-1, 1) + (row sum + 1) I: every step's diagonal pivot is safely away from zero."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, (n, n))
    return a + np.diag(np.abs(a).sum(axis=1) + 1.0)


def dominant_with_zeros(n, seed):
    """About half of the off-diagonal entries exactly 0: many zero multipliers, which the path multiplies through."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, (n, n))
    a[rng.random((n, n)) < 0.5] = 0.0
    np.fill_diagonal(a, 0.0)
    return a + np.diag(np.abs(a).sum(axis=1) + 1.0)


def dominant_row_scaled(n, seed):
    """Rows scaled by powers of two across +-60 in exponent: where the division by the pivot happens matters."""
    rng = np.random.default_rng(seed)
    return dominant(n, seed) * np.ldexp(1.0, rng.integers(-60, 61, n))[:, None]


INPUTS = (dominant, dominant_with_zeros, dominant_row_scaled)


def run(inv, a):
    x, st = inv.inv(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    torch.cuda.synchronize()
    return x.cpu().numpy(), st.cpu().numpy()


def test_dispatch_and_block_width():
    inv = g.Inverter(algo="auto", pivoting=False)
    try:
        for n in (1, 300, 511):
            assert inv.resolved_blocking_f64(n) == 0, n
        for n in (512, 1000, 4096):
            assert inv.resolved_blocking_f64(n) > 0, n
    finally:
        inv.close()
    inv = g.Inverter(algo="sweep", pivoting=False)
    try:
        assert all(inv.resolved_blocking_f64(n) == 0 for n in (1, 100, 512, 4096))
    finally:
        inv.close()
    inv = g.Inverter(algo="blocked", pivoting=False)
    try:
        assert inv.resolved_blocking_f64(100) > 0
    finally:
        inv.close()
    for req, want in ((64, 64), (128, 128), (256, 128)):   # a request maps to 64 or 128
        inv = g.Inverter(algo="auto", pivoting=False, block_width=req)
        try:
            assert inv.resolved_blocking_f64(1024) == want, req
        finally:
            inv.close()


@pytest.mark.parametrize("n", [512, 513, 640, 1000, 1024, 1500, 2048, 3001])
def test_auto_bit_identical_to_oracle(oracle, n):
    invs = {bw: g.Inverter(algo="auto", pivoting=False, block_width=bw) for bw in (64, 128)}
    try:
        for k, make in enumerate(INPUTS):
            a = make(n, 7000 + 10 * n + k)
            want, info = oracle.matrix_inversion_no_pivots(a, n, return_info=True)
            assert info["status"] == 0
            for bw, inv in invs.items():
                assert inv.resolved_blocking_f64(n) == bw
                x, st = run(inv, a)
                assert int(st[0]) == 0, (make.__name__, n, bw)
                assert np.array_equal(x.reshape(-1), want), (make.__name__, n, bw)
    finally:
        for inv in invs.values():
            inv.close()


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 100, 257])
def test_explicit_blocked_small_orders_bit_identical_to_oracle(oracle, n):
    """Orders far from a multiple of the block width: the identity padding."""
    inv = g.Inverter(algo="blocked", pivoting=False)
    try:
        assert inv.resolved_blocking_f64(n) > 0
        for k, make in enumerate(INPUTS):
            a = make(n, 8000 + 10 * n + k)
            want = oracle.matrix_inversion_no_pivots(a, n)
            x, st = run(inv, a)
            assert int(st[0]) == 0 and np.array_equal(x.reshape(-1), want), (make.__name__, n)
    finally:
        inv.close()


def test_batch_members_independent_and_status(oracle):
    """[dominant, row and column 700 zeroed (pivot exactly 0 at step 700, inside a later block), one NaN entry,
    dominant]: status [0, 2, 2, 0] as the oracle's; the regular members as the oracle and as single runs."""
    n = 1000
    a0, a3 = dominant(n, 1), dominant(n, 4)
    a1 = dominant(n, 2)
    a1[700, :] = 0.0
    a1[:, 700] = 0.0
    a2 = dominant(n, 3)
    a2[123, 456] = np.nan
    mats = [a0, a1, a2, a3]
    want_status = [oracle.matrix_inversion_no_pivots(m, n, return_info=True)[1]["status"] for m in mats]
    assert want_status == [0, 2, 2, 0]
    inv = g.Inverter(algo="auto", pivoting=False)
    try:
        x, st = run(inv, np.stack(mats))
        assert st.tolist() == want_status
        for b in (0, 3):
            want = oracle.matrix_inversion_no_pivots(mats[b], n)
            assert np.array_equal(x[b].reshape(-1), want), b
            xs, sts = run(inv, mats[b])
            assert int(sts[0]) == 0 and np.array_equal(xs, x[b]), b
    finally:
        inv.close()


def test_host_entry_points(oracle):
    n = 1024
    a = dominant(n, 1024)
    want = oracle.matrix_inversion_no_pivots(a, n)
    got = g.matrix_inversion_no_pivots(a.reshape(-1), n)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    sing = a.copy()
    sing[700, :] = 0.0
    sing[:, 700] = 0.0
    assert g.matrix_inversion_no_pivots(sing.reshape(-1), n).size == 0
    y, t = g.fp64_bench(a.reshape(-1), n, pivoting=False)
    assert np.array_equal(y, want)
    assert t["pivot"] > 0 and t["column"] > 0   # the diagonal blocks, the block-column / strip / rank-bw updates


def test_profile_has_no_sweep_steps():
    n = 1024
    inv = g.Inverter(algo="auto", pivoting=False)
    try:
        ta = torch.from_numpy(dominant(n, 5)).cuda()
        inv.set_profiling(True)
        inv.get_profile()
        inv.inv(ta)
        prof = inv.get_profile()
        inv.set_profiling(False)
    finally:
        inv.close()
    assert prof["sweep_step"][1] == 0
    assert prof["panel"][1] > 0 and prof["update_rank_bw"][1] > 0


def test_4096_bit_identical_and_faster_than_sweep(oracle):
    n = 4096
    a = dominant(n, 4096)
    want = oracle.matrix_inversion_no_pivots(a, n)
    ta = torch.from_numpy(a).cuda()
    times = {}
    for algo in ("auto", "sweep"):
        inv = g.Inverter(algo=algo, pivoting=False)
        try:
            x, st = inv.inv(ta)   # also the warm-up
            torch.cuda.synchronize()
            assert int(st[0]) == 0
            assert np.array_equal(x.cpu().numpy().reshape(-1), want), algo
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                inv.inv(ta, out=x)
            torch.cuda.synchronize()
            times[algo] = (time.perf_counter() - t0) / 3 * 1e3
        finally:
            inv.close()
    print(f"fp64 no-pivot N=4096: blocked {times['auto']:.2f} ms, sweep {times['sweep']:.2f} ms")
    assert times["auto"] * 5 < times["sweep"]
