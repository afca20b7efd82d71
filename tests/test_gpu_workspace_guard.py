"""GPU tests of what the dense routes do INSIDE the workspace (run with ``-m gpu`` on an MI355X), in the library's
diagnostic guard mode: every carve gets a red zone in front of its first region and one behind every region, the value
regions and the zones behind them hold the quiet NaN 0x7FF8DEAD, the zones behind index and record regions hold zeros.

``guarded`` is the one harness: it sets the guard size, opens a FRESH ``Inverter`` with the case's settings, runs the
call, asks ``mi32_debug_ws_check`` and asserts that as many zones were checked as the layout of the call has regions
plus one per carve (so something really was armed) and that none is damaged (the message names the region and the
offset).  The caller then compares status and result bit for bit with the reference: the route's oracle as
guard_cases.INV_ROUTES names it up to order 1024, the same call on a second context with the guard off above (other
tests hold that result to the oracle).  Values and zones being poisoned, bit equality also shows that no result depends
on workspace the call did not write.  There is no tolerance in this file.

The guard size is max(64 KiB, two rows of the route's widest padded row), so a stray row cannot jump a zone.  What the
mode cannot see is listed in DESIGN.md ("Ordering and workspace contract").
"""
import numpy as np
import pytest

import guard_cases as GC
import residual_cases
import workspace_cases as W
from conftest import gate_matrix
from nopivot_cases import spd

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_matrix_inversion_amd as g  # noqa: E402
from gpu_matrix_inversion_amd import _lib  # noqa: E402

F32, F64 = W.F32, W.F64
OK = 0


@pytest.fixture(scope="module")
def lib():
    lib = W.bind(_lib.load())
    try:
        yield lib
    finally:
        assert lib.mi32_debug_ws_guard(0) == 0


# ---- inputs and references, built once per module ------------------------------------------------------------------------
_MATS, _WANT = {}, {}


def matrix(pivoting, dtype, n, b=0):
    key = (pivoting, np.dtype(dtype).name, n, b)
    if key not in _MATS:
        seed = 9500 + 13 * n + b
        a = gate_matrix(n, seed).astype(dtype) if pivoting else spd(n, seed, dtype)
        a.setflags(write=False)
        _MATS[key] = a
    return _MATS[key]


def batch_of(pivoting, dtype, n, members, distinct=None):
    distinct = members if distinct is None else distinct
    return np.stack([matrix(pivoting, dtype, n, b % distinct) for b in range(members)])


def oracle_inverse(oracle, pivoting, dtype, n, b, ref, bw=None):
    """The (n, n) inverse of ``matrix(pivoting, dtype, n, b)`` on the reference ``ref`` of guard_cases; its status is OK."""
    key = (pivoting, np.dtype(dtype).name, n, b, ref, bw)
    if key not in _WANT:
        a = matrix(pivoting, dtype, n, b)
        if ref == "mirror64":
            assert dtype == F64 and pivoting and bw
            x, info = oracle.matrix_inv_64_blocked(a, n, bw, return_info=True)
        else:
            fn = (oracle.matrix_inversion_no_pivots if not pivoting else
                  oracle.matrix_inv_32_inplace if dtype == F32 else oracle.matrix_inv_64)
            x, info = fn(a, n, return_info=True, zeros={"steps": "skip", "through": "through"}[ref])
        x = np.ascontiguousarray(x.reshape(n, n))
        assert int(info["status"]) == OK and x.dtype == dtype and np.isfinite(x).all()
        x.setflags(write=False)
        _WANT[key] = x
    return _WANT[key]


# ---- the harness ---------------------------------------------------------------------------------------------------------
def open_inverter(c):
    return g.Inverter(algo=c.algo, pivoting=c.pivoting, **c.knobs)


def row_bytes(lib, handle, n, batch, es):
    """Bytes of the widest padded row the route's kernels step by: the multiplier panels of blocked fp32 (2 np + 256
    floats), the working copies elsewhere."""
    r = W.dense_route(lib, handle, n, batch, es)
    if r["path"] == W.BLOCKED32:
        return (2 * r["np"] + 256) * 4
    return (r["np"] if r["np"] else (n + 3) & ~3) * es


def guarded(lib, c, n, batch, es, call, owners=(W.INVERSE,), inv=None):
    """``call(inv)`` on a fresh Inverter of case ``c`` (or on ``inv``) in guard mode; the zones are checked before the
    Inverter is closed.  Returns what ``call`` returned, as numpy arrays."""
    G = W.guard_bytes(row_bytes(lib, None if inv is None else inv._h, n, batch, es))
    own = inv is None
    with W.guard(lib, G) as size:
        assert size == G and G >= 65536
        inv = open_inverter(c) if own else inv
        try:
            carves = [regs for (owner, _), regs in W.carves(W.layout(lib, inv._h, n, batch, es)) if owner in owners]
            out = call(inv)
            torch.cuda.synchronize()
            r = W.check(lib, inv._h)
            assert r.checked == sum(len(regs) + 1 for regs in carves), (c, r.checked, [len(x) for x in carves])
            assert r.checked > 0 or not carves
            assert r.damaged == 0, (c, W.describe(r))
            return tuple(None if t is None else t.cpu().numpy() for t in out)
        finally:
            if own:
                inv.close()


def unguarded(lib, c, call):
    """The same call on a second context with the guard off."""
    assert lib.mi32_debug_ws_guard(0) == 0
    inv = open_inverter(c)
    try:
        out = call(inv)
        torch.cuda.synchronize()
        assert W.check(lib, inv._h).checked == 0   # nothing is armed with the guard off
        return tuple(None if t is None else t.cpu().numpy() for t in out)
    finally:
        inv.close()


def assert_inverse(oracle, lib, c, mats, got, status, distinct=None):
    batch, n = mats.shape[0], mats.shape[1]
    assert status.tolist() == [OK] * batch, (c.name, status)
    if n <= W.ORACLE_MAX:
        bw = None
        if c.reference == "mirror64":
            bw64 = W.dense_route(lib, None, n, batch, 8)["bw"]
            assert bw64 > 0
            bw = bw64
        for b in range(batch):
            want = oracle_inverse(oracle, c.pivoting, c.dtype, n, b % (distinct or batch), c.reference, bw)
            assert GC.same_bits(got[b], want), (c.name, "member", b, GC.first_difference(got[b], want))
    else:
        d = torch.from_numpy(mats).cuda()
        want, st = unguarded(lib, c, lambda inv: inv.inv(d))
        assert st.tolist() == [OK] * batch and np.isfinite(want).all()
        assert GC.same_bits(got, want), (c.name, GC.first_difference(got, want))


def set_env(monkeypatch, c):
    for name, value in c.env.items():
        monkeypatch.setenv(name, value)


# ---- every route ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", W.INV_CASES, ids=[c.name for c in W.INV_CASES])
def test_inverse_in_a_guarded_workspace(oracle, lib, monkeypatch, c):
    set_env(monkeypatch, c)
    es = np.dtype(c.dtype).itemsize
    mats = batch_of(c.pivoting, c.dtype, c.n, c.batch)
    d = torch.from_numpy(mats).cuda()
    route = W.dense_route(lib, None, c.n, c.batch, es)
    if c.reference == "mirror64":
        assert route["path"] == W.BLOCKED64 and (not c.env or route["bw"] == min(int(c.env["MI32_BLOCK_W64"]),
                                                                                  -(-c.n // 64) * 64))
    x, st = guarded(lib, c, c.n, c.batch, es, lambda inv: inv.inv(d))
    assert_inverse(oracle, lib, c, mats, x, st)


def test_blocked_fp32_in_two_parts(oracle, lib):
    """guard_cases' split shape: both carves are armed and checked, the second where the first ends."""
    n, batch, distinct = GC.SPLIT_ORDER, GC.SPLIT_BATCH, GC.SPLIT_DISTINCT
    c = W.Case("blocked32-split", "blocked", True, F32, n, batch, "through")
    assert _lib.resolve_route(None, n, batch)[0]["parts"] == 2
    mats = batch_of(True, F32, n, batch, distinct)
    d = torch.from_numpy(mats).cuda()
    with W.guard(lib, 65536):
        parts = W.carves(W.layout(lib, None, n, batch, 4), W.INVERSE)
    assert [key for key, _ in parts] == [(W.INVERSE, 0), (W.INVERSE, 1)]
    x, st = guarded(lib, c, n, batch, 4, lambda inv: inv.inv(d))
    assert_inverse(oracle, lib, c, mats, x, st, distinct)


# ---- the determinant beside the inverse ----------------------------------------------------------------------------------
@pytest.mark.parametrize("d", GC.DET_ANY, ids=[f"{d.name}-{d.n}" for d in GC.DET_ANY])
def test_inv_det_any_in_guarded_memory(oracle, lib, d):
    """The det memory's zones are checked beside the workspace's; inverse, status and pair equal the unguarded call's
    bit for bit and the inverse the oracle's.  (The wide row runs a one-launch kernel, which carves nothing: no zone.)"""
    c = W.Case(d.name, d.algo, d.pivoting, d.dtype, d.n, 1, d.reference)
    es = np.dtype(d.dtype).itemsize
    mats = batch_of(d.pivoting, d.dtype, d.n, 1)
    dev = torch.from_numpy(mats).cuda()
    one_launch = d.name == "wide"
    want = unguarded(lib, c, lambda inv: inv.inv_det_any(dev))
    got = guarded(lib, c, d.n, 1, es, lambda inv: inv.inv_det_any(dev), owners=() if one_launch else (W.INVERSE, W.DET))
    for a, b, what in zip(got, want, ("inverse", "status", "det_mant", "det_exp")):
        assert GC.same_bits(a, b), (d.name, what, GC.first_difference(a, b))
    assert np.isfinite(got[2]).all() and (np.abs(got[2]) >= 0.5).all() and (np.abs(got[2]) < 1.0).all()
    assert_inverse(oracle, lib, c, mats, got[0], got[1])
    # the determinant-only form carves the same
    got = guarded(lib, c, d.n, 1, es, lambda inv: inv.inv_det_any(dev, want_inverse=False),
                  owners=() if one_launch else (W.INVERSE, W.DET))
    assert got[0] is None and GC.same_bits(got[2], want[2]) and GC.same_bits(got[3], want[3]), d.name


# ---- the residual verifier -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", W.RESIDUAL_ORDERS)
def test_residual_in_a_guarded_workspace(lib, n):
    """Exact integer operands (residual_cases.integer_batch): the two norms equal the int64 answer and all three numbers
    the unguarded call's, bit for bit."""
    c = W.Case("residual", "auto", True, F32, n, W.RESIDUAL_BATCH, None)
    a, x = residual_cases.integer_batch(n, W.RESIDUAL_BATCH, 6200)
    da, dx = torch.from_numpy(a).cuda(), torch.from_numpy(x).cuda()
    want, = unguarded(lib, c, lambda inv: (inv.residual(da, dx),))
    got, = guarded(lib, c, n, W.RESIDUAL_BATCH, 4, lambda inv: (inv.residual(da, dx),), owners=(W.RESIDUAL,))
    assert got.shape == (W.RESIDUAL_BATCH, 3) and np.isfinite(got).all()
    assert GC.same_bits(got, want), (n, got, want)
    assert GC.same_bits(got[:, :2], residual_cases.expected_exact(a, x)[:, :2])


def test_residual_right_behind_a_guarded_inversion(oracle, lib):
    """Queued on the same context with nothing in between: the verifier's carve is armed over the inversion's workspace
    only after the inversion has left it, and the zones reported on are the verifier's.  The inverse is the oracle's all
    the same; the verifier's operands are the exact integer ones, so its numbers compare bit for bit."""
    n, batch = 100, W.RESIDUAL_BATCH
    c = W.Case("blocked32", "blocked", True, F32, n, batch, "through")
    mats = batch_of(True, F32, n, batch)
    d = torch.from_numpy(mats).cuda()
    a, x = residual_cases.integer_batch(n, batch, 6300)
    da, dx = torch.from_numpy(a).cuda(), torch.from_numpy(x).cuda()

    def both(inv):
        return inv.inv(d) + (inv.residual(da, dx),)

    got, st, res = guarded(lib, c, n, batch, 4, both, owners=(W.RESIDUAL,))
    assert_inverse(oracle, lib, c, mats, got, st)
    want, = unguarded(lib, c, lambda inv: (inv.residual(da, dx),))
    assert res.shape == (batch, 3) and GC.same_bits(res, want), (res, want)
    assert GC.same_bits(res[:, :2], residual_cases.expected_exact(a, x)[:, :2])


# ---- two calls on one guarded context ------------------------------------------------------------------------------------
def test_check_reports_on_the_last_call_only(oracle, lib):
    """Blocked fp32 at 300 (31 zones), then the fp64 sweep at 100 (7 zones) in the same, larger workspace."""
    big = W.Case("blocked32", "auto", True, F32, 300, 1, "through")
    small = W.Case("sweep64", "auto", True, F64, 100, 1, "steps")
    a, b = batch_of(True, F32, 300, 1), batch_of(True, F64, 100, 1)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    assert W.dense_route(lib, None, 300, 1, 4)["path"] == W.BLOCKED32
    assert W.dense_route(lib, None, 100, 1, 8)["path"] == W.SWEEP
    inv = open_inverter(big)
    try:
        x, st = guarded(lib, big, 300, 1, 4, lambda i: i.inv(da), inv=inv)
        assert W.check(lib, inv._h).checked == len(W.BLOCKED32_REGIONS) + 1
        y, st2 = guarded(lib, small, 100, 1, 8, lambda i: i.inv(db), inv=inv)
        r = W.check(lib, inv._h)
        assert (r.checked, r.damaged) == (len(W.REGIONS[W.SWEEP]) + 1, 0), W.describe(r)
    finally:
        inv.close()
    assert_inverse(oracle, lib, big, a, x, st)
    assert_inverse(oracle, lib, small, b, y, st2)


# ---- the checker itself --------------------------------------------------------------------------------------------------
def test_the_checker_sees_one_poked_word(lib):
    """After a clean call, one word stored into the first, a middle and the last zone: exactly that zone, that offset
    and 4 bytes; the word put back, the zones are clean again.  An offset outside the zone is refused."""
    n = 130
    c = W.Case("blocked32", "blocked", True, F32, n, 1, "through")
    d = torch.from_numpy(batch_of(True, F32, n, 1)).cuda()
    G = W.guard_bytes(row_bytes(lib, None, n, 1, 4))
    names = W.BLOCKED32_REGIONS
    inv = open_inverter(c)
    try:
        guarded(lib, c, n, 1, 4, lambda i: i.inv(d), inv=inv)
        zones = len(names) + 1
        for zone, offset in ((0, 0), (0, G - 4), (8, 1028), (zones - 1, 0), (zones - 1, G - 4)):
            region = names[max(zone - 1, 0)]                       # zone 0 leads, zone k lies behind region k - 1
            pattern = W.POISON if W.KIND_OF[region] == W.VALUES else 0
            assert lib.mi32_debug_ws_poke(inv._h, zone, offset, W.POKE) == 0
            r = W.check(lib, inv._h)
            assert (r.checked, r.damaged, r.zone, r.owner, r.part) == (zones, 1, zone, W.INVERSE, 0), W.describe(r)
            assert (r.name.decode(), r.offset, r.bytes) == (region, offset - G if zone == 0 else offset, 4), W.describe(r)
            assert lib.mi32_debug_ws_poke(inv._h, zone, offset, pattern) == 0
            r = W.check(lib, inv._h)
            assert (r.checked, r.damaged, r.bytes, r.name) == (zones, 0, 0, b""), W.describe(r)
        for zone, offset in ((0, G), (0, -4), (0, 2), (3, G - 2), (zones, 0), (-1, 0)):
            assert lib.mi32_debug_ws_poke(inv._h, zone, offset, W.POKE) != 0, (zone, offset)
        assert W.check(lib, inv._h).damaged == 0
    finally:
        inv.close()
