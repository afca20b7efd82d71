"""GPU tests of the pivoted fp64 inversion (matrix_inversion_FP64 of the reference): the blocked path of
mi32_blocked64.hip (from N = 256 on) and the sweep of mi32_sweep.hip on double (below, or with algo="sweep").

What is pinned here, bit for bit against the CPU mirrors (oracle.matrix_inv_64_blocked for the blocked path at its
block width, oracle.matrix_inv_64 for the sweep), all through Inverter.inv on torch.float64 tensors:
  * the 32-rows-per-workgroup geometry of the step and prep kernels, which every order above 4096 runs;
  * batches by value on both paths: every member against the mirror of that member alone, in both member orders;
  * exact ties of the two-word arg-max record (tests/fp64_cases.py: inside a row tile, across tiles, across the two
    turns of the record loop above 256 records, at the seam where the records come from the prep kernel, in the
    second column tile of the sweep);
  * input unchanged, out=, one handle across shapes.
And against a reference that shares nothing with the elimination (fp64_cases.reference_inverse: numpy's inverse
polished in extended precision): forward error within kappa_inf 2^-53, residual within 4 n kappa_inf 2^-53.

Not asserted here: the residual of the fp64 blocked path against the reference-order oracle's.  Its rank-bw update
is still the composite order, and on `rand` at N = 2048 its ||A X - I||_inf is about 3.5 x that
of the reference-order elimination; these tests are what a move to the reference's order will be held to.
"""
import functools

import numpy as np
import pytest

import fp64_cases as C
from degenerate_cases import zero_row

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_matrix_inversion_amd as g  # noqa: E402

needs_extended = pytest.mark.skipif(not C.longdouble_is_extended(), reason="np.longdouble is not an extended format")


def _inverter_fixture(**kw):
    @pytest.fixture(scope="module")
    def fx():
        inv = g.Inverter(**kw)
        try:
            yield inv
        finally:
            inv.close()
    return fx


inv_auto = _inverter_fixture(algo="auto")                       # blocked from N = 256 on, bw 128
inv_bw64 = _inverter_fixture(algo="auto", block_width=64)
inv_bw256 = _inverter_fixture(algo="auto", block_width=256)
inv_sweep = _inverter_fixture(algo="sweep")


def run(inv, a, **kw):
    """(inverse, status) as numpy arrays; the input must come back bit-unchanged."""
    a = np.array(a, dtype=np.float64)   # a writable copy: the shared inputs are read-only
    ta = torch.from_numpy(a).cuda()
    x, st = inv.inv(ta, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(ta.cpu().numpy(), a), "the input tensor was modified"
    return x.cpu().numpy(), st.cpu().numpy()


def assert_same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want).reshape(np.shape(got))
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist())


# ---- 1. the 32-row geometry above 4096 rows ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tall_input():
    n = 4100
    a = C.dist_matrix64("gate", n, 64_4100)
    x = np.linalg.inv(a)
    a.setflags(write=False)
    return a, float(C.norm_inf(a) * C.norm_inf(x))


@pytest.mark.parametrize("bw_req,bw,padded", [(0, 128, 4224), (64, 64, 4160), (256, 256, 4352)])
def test_tall_geometry_above_4096_rows_bit_identical_to_mirror(oracle, inv_auto, inv_bw64, inv_bw256, bw_req, bw, padded):
    """N = 4100: more than 4096 padded rows, so the plan takes 32 rows per workgroup -- b64_panel_step_kernel<32,32>,
    <16,32>, <64,32> (4, 2, 8 row passes per thread) and the 32-row form of the prep kernel."""
    n = 4100
    a, kappa = _tall_input()
    inv = {0: inv_auto, 64: inv_bw64, 256: inv_bw256}[bw_req]
    assert inv.resolved_blocking_f64(n) == bw and -(-n // bw) * bw == padded and padded > 4096
    ta = torch.from_numpy(a.copy()).cuda()
    x, st = inv.inv(ta)
    res = float((ta @ x - torch.eye(n, dtype=torch.float64, device="cuda")).abs().sum(dim=1).max())
    torch.cuda.synchronize()
    assert int(st[0]) == 0
    # the independent check first: its message says how wrong, the bit comparison only where
    bound = 4 * n * kappa * C.U64
    print(f"N={n} bw={bw}: ||A X - I||_inf {res:.3e}, bound {bound:.3e} (kappa_inf {kappa:.3e})")
    assert res <= bound, res / bound
    want, info = oracle.matrix_inv_64_blocked(a, n, bw, return_info=True)
    assert info["status"] == 0
    assert_same_bits(x.cpu().numpy(), want, (n, bw))
    assert np.array_equal(ta.cpu().numpy(), a), "the input tensor was modified"


# ---- 2. batches by value, blocked ----------------------------------------------------------------------------------
def _blocked_batch_members(n):
    late = C.dist_matrix64("gate", n, 64_304)
    late[n - 1] = late[n - 2]          # singular in exact arithmetic, noticed (if at all) by the last steps
    return [C.dist_matrix64("gate", n, 64_301), C.dist_matrix64("ref100", n, 64_302),
            C.dist_matrix64("hollow", n, 64_303), late]


@pytest.mark.parametrize("bw_req", [0, 64])
def test_blocked_batch_by_value_both_member_orders(oracle, inv_auto, inv_bw64, bw_req):
    """B = 4, N = 300: every member is the mirror of that member alone and the single-matrix call of the same
    inverter, whatever slot it sits in -- the per-member offsets of records, row maps and working copies."""
    n = 300
    inv = inv_auto if bw_req == 0 else inv_bw64
    bw = inv.resolved_blocking_f64(n)
    assert bw == (128 if bw_req == 0 else 64)
    members = _blocked_batch_members(n)
    mirror = [oracle.matrix_inv_64_blocked(m, n, bw, return_info=True) for m in members]
    assert [info["status"] for _, info in mirror[:3]] == [0, 0, 0]
    single = [run(inv, m) for m in members]
    for order in ([0, 1, 2, 3], [3, 2, 1, 0]):
        batch = np.stack([members[i] for i in order])
        got, st = run(inv, batch)
        out = torch.full((4, n, n), np.nan, dtype=torch.float64, device="cuda")
        got_out, st_out = run(inv, batch, out=out)
        assert_same_bits(out.cpu().numpy(), got_out, ("out= is not what was returned", order))
        for slot, i in enumerate(order):
            want, info = mirror[i]
            assert st[slot] == st_out[slot] == single[i][1][0] == info["status"], (order, slot)
            if info["status"] == 0:
                assert_same_bits(got[slot], want, ("mirror", order, slot))
                assert_same_bits(got[slot], single[i][0], ("single call", order, slot))
                assert_same_bits(got_out[slot], want, ("out=", order, slot))


def test_blocked_batch_flags_a_singular_member_only(oracle, inv_auto):
    """The same batch shape with a member that IS status 2 on the mirror (a zero row loses every search: the zero
    pivot comes at the last step), in a middle slot: flagged there and nowhere else, the others untouched."""
    n = 300
    members = _blocked_batch_members(n)[:3]
    members.insert(2, zero_row(n, 100, 64_305, np.float64))
    bw = inv_auto.resolved_blocking_f64(n)
    got, st = run(inv_auto, np.stack(members))
    want = [oracle.matrix_inv_64_blocked(m, n, bw, return_info=True) for m in members]
    assert [info["status"] for _, info in want] == [0, 0, 2, 0] == st.tolist()
    for b in (0, 1, 3):
        assert_same_bits(got[b], want[b][0], b)


# ---- 3. batches by value, sweep --------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,n", [(5, 70), (3, 257)])
def test_sweep_batch_by_value(oracle, inv_sweep, batch, n):
    kinds = ["gate", "ref100", "hollow", "rand", "gate"][:batch]
    members = [C.dist_matrix64(k, n, 64_500 + n + b) for b, k in enumerate(kinds)]
    mid = batch // 2
    members[mid] = zero_row(n, n // 3, 64_600 + n, np.float64)
    want = [oracle.matrix_inv_64(m, n, return_info=True) for m in members]
    assert [info["status"] for _, info in want] == [2 if b == mid else 0 for b in range(batch)]
    for order in (list(range(batch)), list(range(batch))[::-1]):
        got, st = run(inv_sweep, np.stack([members[i] for i in order]))
        assert st.tolist() == [want[i][1]["status"] for i in order]
        for slot, i in enumerate(order):
            if i != mid:
                assert_same_bits(got[slot], want[i][0], (order, slot))


# ---- 4. sweep above one column tile and above 256 records -------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gate", "ref100", "ties"])
def test_sweep_1100_two_column_tiles_275_records(oracle, inv_sweep, kind):
    """N = 1100 on the fp64 sweep: two column tiles (the pivot columns from 1024 on and their records belong to the
    second), 275 row tiles of 4 rows, so the record loop takes a second turn; with ties 1, 4 and 1024 rows apart and
    tie columns beyond 1024."""
    n = 1100
    a = C.tie_case("s1100")[0] if kind == "ties" else C.dist_matrix64(kind, n, 64_700 + len(kind))
    want, info = oracle.matrix_inv_64(a, n, return_info=True)
    got, st = run(inv_sweep, a)
    assert st[0] == info["status"] == 0
    assert_same_bits(got, want, kind)


# ---- 5. ties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bw_req", [64, 0])
def test_blocked_ties_short_range(oracle, inv_auto, inv_bw64, bw_req):
    a, _ = C.tie_case("t300")
    n = a.shape[0]
    inv = inv_auto if bw_req == 0 else inv_bw64
    bw = inv.resolved_blocking_f64(n)
    assert bw == (128 if bw_req == 0 else 64)
    want, info = oracle.matrix_inv_64_blocked(a, n, bw, return_info=True)
    got, st = run(inv, a)
    assert st[0] == info["status"] == 0
    assert_same_bits(got, want, bw)


def test_blocked_ties_2048_rows_apart_across_two_turns_of_the_record_loop(oracle, inv_auto):
    a, _ = C.tie_case("t2100")
    n = a.shape[0]
    assert inv_auto.resolved_blocking_f64(n) == 128 and -(-n // 128) * 128 // 8 == 272
    want, info = oracle.matrix_inv_64_blocked(a, n, 128, return_info=True)
    got, st = run(inv_auto, a)
    assert st[0] == info["status"] == 0
    assert_same_bits(got, want, n)


def test_sweep_ties_short_range(oracle, inv_sweep):
    """The short-range placements on the fp64 sweep as well (TR = 4 at this order: rows 8 | 9 share a tile)."""
    a, _ = C.tie_case("t300")
    n = a.shape[0]
    want, info = oracle.matrix_inv_64(a, n, return_info=True)
    got, st = run(inv_sweep, a)
    assert st[0] == info["status"] == 0
    assert_same_bits(got, want, n)


# ---- 6. the independent reference ------------------------------------------------------------------------------------
@needs_extended
@pytest.mark.parametrize("kind,n", C.REFERENCE_CASES)
def test_forward_error_and_residual_against_the_extended_precision_reference(inv_auto, inv_bw64, inv_bw256, inv_sweep, kind, n):
    """max|X - Xref| / max|Xref| <= kappa_inf 2^-53 and ||A X - I||_inf (longdouble, on the host) <= 4 n kappa_inf 2^-53
    for the blocked path at bw 64, 128 and 256 and, at N = 257 and 300, for the sweep."""
    a, xref = C.reference_case(kind, n)
    bound = C.forward_bound(a, xref)
    rbound = 4 * n * C.kappa_inf(a, xref) * C.U64
    paths = [("bw64", inv_bw64, 64), ("bw128", inv_auto, 128), ("bw256", inv_bw256, 256)]
    if n <= 300:
        paths.append(("sweep", inv_sweep, 0))
    failures = []
    for name, inv, bw in paths:
        assert inv.resolved_blocking_f64(n) == bw
        got, st = run(inv, a)
        assert st[0] == 0, name
        err = C.forward_error(got, xref)
        res = float(C.residual_inf_longdouble(a, got))
        print(f"{kind} N={n} {name}: forward error {err / bound:.3f} of its bound, residual {res / rbound:.2e} of its bound")
        if not (err <= bound and res <= rbound):
            failures.append((name, err / bound, res / rbound))
    assert not failures, failures


# ---- 7. one handle across shapes -------------------------------------------------------------------------------------
def test_one_handle_across_shapes_and_precisions():
    """The workspace of a handle grows and is carved anew per call: N = 700, then 4 x 300, 2 x 100 (sweep), 520, an
    fp32 call, and 700 again on ONE inverter -- each call what a fresh inverter gives, the last the first's bits."""
    def a64(n, batch, seed):
        return torch.from_numpy(np.stack([C.dist_matrix64("gate", n, seed + b) for b in range(batch)])).cuda()

    calls = [a64(700, 1, 64_900), a64(300, 4, 64_910), a64(100, 2, 64_920), a64(520, 1, 64_930),
             a64(300, 1, 64_940).float(), a64(700, 1, 64_900)]
    one = g.Inverter(algo="auto")
    try:
        assert one.resolved_blocking_f64(700) == 128 and one.resolved_blocking_f64(100) == 0
        got = []
        for t in calls:
            x, st = one.inv(t)
            torch.cuda.synchronize()
            got.append((x.clone(), st.clone()))
    finally:
        one.close()
    for k, t in enumerate(calls):
        fresh = g.Inverter(algo="auto")
        try:
            x, st = fresh.inv(t)
            torch.cuda.synchronize()
            assert st.tolist() == [0] * t.shape[0] == got[k][1].tolist(), k
            assert x.dtype == t.dtype and torch.equal(x, got[k][0]), k
        finally:
            fresh.close()
    assert torch.equal(got[0][0], got[-1][0])
