"""GPU tests of WHERE the dense device calls read and write (run with ``-m gpu`` on an MI355X): ``inv``, ``inv_det``,
``inv_det_any``, ``solve`` and ``residual`` are handed views carved out of larger buffers by tests/guard_cases.py, one
element past a 256-byte boundary (element aligned and nothing more; one aligned control per route), with NaN margins
around the inputs and sentinel margins around the outputs, the status words and the determinant pair.

Every case runs a route on ordinary well-conditioned inputs (``gate_matrix`` with pivoting, ``nopivot_cases.spd``
without), so the reference alone decides the values.  There is no tolerance in this file and no route is skipped.  Every
case asserts

  (a) result and status equal the route's reference bit for bit (the references the overflow table names: the step
      oracle for the sweep, the one-launch routes and blocked fp32, ``matrix_inv_64_blocked`` at the resolved width for
      blocked fp64, the no-pivot oracle for the no-pivot routes, the det and solve mirrors for their pairs and ``solve``);
  (b) every margin of the output, the status, ``det_mant`` and ``det_exp`` is intact;
  (c) the input buffers (``a``, and ``b`` unless solved in place) are unchanged bit for bit, NaN margins included;
  (d) first of all, through the ``resolved_*`` queries, that the route the case names is the route that runs.

A load from an input margin would bring a NaN with a payload into (a); a store outside the output shows in (b).

Orders left out for time: none of the issue's list.  The one blocked fp32 shape that runs as two parts is the smallest
there is: a split needs 64 Mi elements, which 1024 members of order 256 (the order that needs no padding) are.

The refusals of ``api.check_dense_args`` are repeated here through a live ``Inverter``; each is followed by a valid call
on the same handle that must give the oracle's bits.
"""
import ctypes

import numpy as np
import pytest

import guard_cases as G
import residual_cases
from conftest import gate_matrix
from det_cases import build_mirror, expected
from det_large_cases import build_mirror_large, expected_pair, mirror_blocked64, mirror_steps
from nopivot_cases import spd
from solve_cases import build_solve_mirror, cap, mirror_solve_batch, rhs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_matrix_inversion_amd as g  # noqa: E402

F32, F64, I32 = G.F32, G.F64, G.I32
OK = 0
LEADS = (G.LEAD_ODD, G.LEAD_ALIGNED)


def dt_id(dtype):
    return "fp32" if dtype == F32 else "fp64"


# ---- inputs and references, computed once --------------------------------------------------------------------------------
_MATS, _WANT = {}, {}


def matrix(pivoting, dtype, n, b=0):
    key = (pivoting, dtype, n, b)
    if key not in _MATS:
        seed = 9000 + 17 * n + b
        a = gate_matrix(n, seed).astype(dtype) if pivoting else spd(n, seed, dtype)
        a.setflags(write=False)
        _MATS[key] = a
    return _MATS[key]


def batch_of(pivoting, dtype, n, members):
    return np.stack([matrix(pivoting, dtype, n, b) for b in range(members)])


def reference(oracle, pivoting, dtype, n, b, ref, bw=None):
    """(inverse (n, n), status) of ``matrix(pivoting, dtype, n, b)`` on the reference ``ref`` of guard_cases."""
    key = (pivoting, dtype, n, b, ref, bw)
    if key not in _WANT:
        a = matrix(pivoting, dtype, n, b)
        if ref == "mirror64":
            assert dtype == F64 and pivoting and bw
            x, info = oracle.matrix_inv_64_blocked(a, n, bw, return_info=True)
        else:
            zeros = {"steps": "skip", "through": "through"}[ref]
            fn = (oracle.matrix_inversion_no_pivots if not pivoting else
                  oracle.matrix_inv_32_inplace if dtype == F32 else oracle.matrix_inv_64)
            x, info = fn(a, n, return_info=True, zeros=zeros)
        x = np.ascontiguousarray(x.reshape(n, n))
        assert x.dtype == dtype and np.isfinite(x).all()
        x.setflags(write=False)
        _WANT[key] = (x, int(info["status"]))
    return _WANT[key]


# ---- handles and mirrors -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inverters():
    """``get(algo, pivoting)``: one handle per setting, made on first use."""
    made = {}

    def get(algo="auto", pivoting=True):
        if (algo, pivoting) not in made:
            made[(algo, pivoting)] = g.Inverter(algo=algo, pivoting=pivoting)
        return made[(algo, pivoting)]

    yield get
    torch.cuda.synchronize()
    for inv in made.values():
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


# ---- guarded buffers on the device ---------------------------------------------------------------------------------------
class Guarded:
    """A buffer of guard_cases.carve on the device: ``host`` (the flat array as it was uploaded), ``whole`` and ``view``
    (device tensors), ``fill``."""

    def __init__(self, shape, dtype, lead, fill, margin, content=None):
        self.host, view = G.carve(shape, dtype, lead, fill, margin)
        if content is not None:
            view[...] = content
        self.span = G.span(self.host, view)
        self.fill, self.shape, self.lead = fill, tuple(shape), lead
        self.whole = torch.from_numpy(self.host).cuda()
        off, size = self.span
        self.view = self.whole[off:off + size].view(self.shape)
        es = self.host.itemsize
        assert self.whole.data_ptr() % 256 == 0 and self.view.is_contiguous()
        assert self.view.data_ptr() % 16 == (es if lead == G.LEAD_ODD else 0)      # element aligned and nothing more

    @property
    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def back(self):
        """The whole buffer as it is on the device now, and its view."""
        now = self.whole.cpu().numpy()
        off, size = self.span
        return now, now[off:off + size].reshape(self.shape)

    def assert_margins(self, tag):
        now, view = self.back()
        r = G.intact(now, self.span, self.fill)
        assert r.ok, (tag, "a margin was written", r, self.shape, self.lead)
        return view

    def assert_unchanged(self, tag):
        now, _ = self.back()
        assert G.same_bits(now, self.host), (tag, "the buffer was written", G.first_difference(now, self.host), self.span)


def inputs(mats, lead, cols=None):
    n = mats.shape[1]
    return Guarded(mats.shape, mats.dtype, lead, G.NAN_IN[mats.dtype.type], G.margin_for(n, cols), mats)


def outputs(shape, dtype, lead, cols=None):
    return Guarded(shape, dtype, lead, G.SENTINEL[np.dtype(dtype).type], G.margin_for(shape[1], cols))


def words(batch, dtype, lead):
    return Guarded((batch,), dtype, lead, G.SENTINEL[np.dtype(dtype).type], G.WORD_MARGIN)


def guarded_inverse(inv, mats, lead, tag, stem=None, want_inverse=True, null_status=False):
    """One dense call on carved buffers.  ``stem`` None: ``Inverter.inv`` with ``out=`` and ``status=``; otherwise the C
    entry point of that name (``_f64`` appended for float64), with a carved determinant pair where it takes one.
    Asserts (b) and (c); returns ``(inverse or None, status or None, det_mant or None, det_exp or None)``."""
    batch, n = mats.shape[0], mats.shape[1]
    a = inputs(mats, lead)
    out = outputs(mats.shape, mats.dtype, lead)
    st = words(batch, I32, lead)
    det = stem is not None and "det" in stem
    mant, exp = (words(batch, F64, lead), words(batch, I32, lead)) if det else (None, None)
    if stem is None:
        x, s = inv.inv(a.view, out=out.view, status=st.view)
        assert x.data_ptr() == out.view.data_ptr() and s.data_ptr() == st.view.data_ptr() and x.shape == mats.shape
    else:
        inv._bind_stream()
        fn = getattr(inv._lib, stem + ("" if mats.dtype == F32 else "_f64"))
        rc = fn(inv._h, a.ptr, n, batch, out.ptr if want_inverse else None, None if null_status else st.ptr,
                *((mant.ptr, exp.ptr) if det else ()))
        assert rc == g.MI32_OK, (tag, rc)
    torch.cuda.synchronize()
    a.assert_unchanged((tag, "a"))
    if want_inverse:
        x = out.assert_margins((tag, "out"))
    else:
        out.assert_unchanged((tag, "out with want_inverse=False"))
        x = None
    if null_status:
        st.assert_unchanged((tag, "status, not passed"))
        s = None
    else:
        s = st.assert_margins((tag, "status"))
    if det:
        return x, s, mant.assert_margins((tag, "det_mant")), exp.assert_margins((tag, "det_exp"))
    return x, s, None, None


def assert_members(oracle, got, status, pivoting, dtype, n, ref, bw, tag, index=None):
    batch = got.shape[0]
    if status is not None:
        assert status.dtype == I32 and status.tolist() == [OK] * batch, (tag, status)
    for b in range(batch):
        want, st_want = reference(oracle, pivoting, dtype, n, b if index is None else index[b], ref, bw)
        assert st_want == OK
        assert G.same_bits(got[b], want), (tag, "member", b, G.first_difference(got[b], want))


def assert_route(inv, route, dtype, n, batch):
    """(d): what the resolved_* queries answer for this shape on this handle."""
    es = np.dtype(dtype).itemsize
    if route.blocked64 and dtype == F64:
        bw = inv.resolved_blocking_f64(n)
        assert bw > 0, (route.name, n, bw)
        return bw
    assert inv.resolved_algo(n, batch) == getattr(g, route.expect), (route.name, n, batch)
    if dtype == F64:
        assert inv.resolved_blocking_f64(n) == 0
    if route.expect == "ALGO_RESIDENT":
        assert inv.resolved_resident(n, es)[0] in (8, 16, 32, 64)
    elif route.expect == "ALGO_WORKGROUP":
        assert inv.resolved_workgroup(n, es)[0] == 256
    elif route.expect == "ALGO_WIDE":
        assert inv.resolved_wide(n, es)[0] in (768, 1024)
    return None


# ---- the plain inverse on every route ------------------------------------------------------------------------------------
INV_CASES = [pytest.param(r, dt, n, id=f"{r.name}-{dt_id(dt)}-{n}") for r in G.INV_ROUTES for dt in r.dtypes
             for n in r.orders]


@pytest.mark.parametrize("route,dtype,n", INV_CASES)
def test_inverse(oracle, inverters, route, dtype, n):
    """Every batch of the route's table at the odd lead; the aligned control at the route's first order.  "tail": one
    member more than fill a workgroup of the one-launch kernel (256 threads, ``resolved_resident`` lanes per member)."""
    inv = inverters(route.algo, route.pivoting)
    es = np.dtype(dtype).itemsize
    for batch in route.batches:
        if batch == "tail":
            lanes = inv.resolved_resident(n, es)[0]
            batch = G.tail_batch(lanes)
            assert batch * lanes > G.RESIDENT_THREADS >= (batch - 1) * lanes
        bw = assert_route(inv, route, dtype, n, batch)
        mats = batch_of(route.pivoting, dtype, n, batch)
        for lead in LEADS if n == route.orders[0] else LEADS[:1]:
            tag = (route.name, dt_id(dtype), n, batch, lead)
            x, st, _, _ = guarded_inverse(inv, mats, lead, tag)
            assert_members(oracle, x, st, route.pivoting, dtype, n, route.reference, bw, tag)


def test_blocked_fp32_in_two_parts(oracle, inverters):
    """1024 x 256^2: the second half's ``d_a`` and ``d_inv`` are offset by 512 members.  Four distinct matrices in turn."""
    n, batch, distinct = G.SPLIT_ORDER, G.SPLIT_BATCH, G.SPLIT_DISTINCT
    inv = inverters("blocked", True)
    route = inv.resolved_route(n, batch)[0]
    assert inv.resolved_algo(n, batch) == g.ALGO_BLOCKED
    assert route["parts"] == 2 and route["part_batch"] == [batch // 2, batch // 2] and route["np"] == n, route
    index = [b % distinct for b in range(batch)]
    mats = batch_of(True, F32, n, distinct)[index]
    tag = ("blocked32 split", n, batch)
    x, st, _, _ = guarded_inverse(inv, mats, G.LEAD_ODD, tag)
    assert st.tolist() == [OK] * batch
    x = x.reshape(batch // distinct, distinct, n, n)
    for b in range(distinct):
        want, st_want = reference(oracle, True, F32, n, b, "through")
        assert st_want == OK
        same = (G.bits_of(x[:, b]) == G.bits_of(want)[None]).all(axis=(1, 2))
        assert same.all(), (tag, "members", (np.flatnonzero(~same)[:8] * distinct + b).tolist())


def test_the_guard_sees_a_member_too_many(inverters):
    """The apparatus itself, on the device: the C entry point is told of one member more than the views hold (the
    margins hold two, so nothing leaves the buffers).  With a valid fourth matrix behind ``a``, the stray member's
    stores are found just behind ``out`` and ``status``, located and counted; with ``a`` ending where it should, the
    stray member's loads meet the NaN margin and its status word says so."""
    n, batch = 9, 3
    inv = inverters("workgroup", True)
    mats = batch_of(True, F32, n, batch + 1)
    assert G.margin_for(n) >= 2 * n * n and G.WORD_MARGIN >= 2
    inv._bind_stream()
    a, out, st = inputs(mats, G.LEAD_ODD), outputs((batch, n, n), F32, G.LEAD_ODD), words(batch, I32, G.LEAD_ODD)
    assert inv._lib.mi32_inv_device(inv._h, a.ptr, n, batch + 1, out.ptr, st.ptr) == g.MI32_OK
    torch.cuda.synchronize()
    a.assert_unchanged("a")
    now, _ = out.back()
    assert G.intact(now, out.span, out.fill) == (False, batch * n * n, n * n)
    now, view = st.back()
    assert G.intact(now, st.span, st.fill) == (False, batch, 1) and view.tolist() == [OK] * batch
    assert now[st.span[0] + batch] == OK
    a, out, st = inputs(mats[:batch], G.LEAD_ODD), outputs(mats.shape, F32, G.LEAD_ODD), words(batch + 1, I32, G.LEAD_ODD)
    assert inv._lib.mi32_inv_device(inv._h, a.ptr, n, batch + 1, out.ptr, st.ptr) == g.MI32_OK
    torch.cuda.synchronize()
    a.assert_unchanged("a")
    out.assert_margins("out")
    assert st.assert_margins("status").tolist() == [OK] * batch + [g.MI32_SINGULAR]


# ---- the determinant beside the inverse ----------------------------------------------------------------------------------
def assert_pair(mant, exp, want_m, want_e, tag):
    want_m, want_e = np.atleast_1d(np.asarray(want_m, F64)), np.atleast_1d(np.asarray(want_e, I32))
    assert np.isfinite(want_m).all() and (np.abs(want_m) >= 0.5).all() and (np.abs(want_m) < 1.0).all(), tag
    assert G.same_bits(mant, want_m) and G.same_bits(exp, want_e), (tag, mant, want_m, exp, want_e)


@pytest.mark.parametrize("dtype", [F32, F64], ids=dt_id)
@pytest.mark.parametrize("pivoting", [True, False], ids=["pivot", "nopivot"])
@pytest.mark.parametrize("n", G.DET_ORDERS)
def test_inv_det(oracle, det_dll, inverters, n, pivoting, dtype):
    """Three members through ``mi32_inv_det_device*`` with a carved pair, with the inverse and without."""
    inv, batch, es = inverters("workgroup", pivoting), 3, np.dtype(dtype).itemsize
    assert inv.resolved_algo(n, batch) == (g.ALGO_RESIDENT if n <= 64 else g.ALGO_WORKGROUP)
    assert (inv.resolved_resident(n, es)[0] > 0) if n <= 64 else (inv.resolved_workgroup(n, es)[0] == 256)
    mats = batch_of(pivoting, dtype, n, batch)
    _, want_st, want_m, want_e = expected(det_dll, mats, pivoting)
    assert want_st.tolist() == [OK] * batch
    for lead, want_inverse in ((G.LEAD_ODD, True), (G.LEAD_ODD, False), (G.LEAD_ALIGNED, True)):
        tag = ("inv_det", dt_id(dtype), n, pivoting, lead, want_inverse)
        x, st, mant, exp = guarded_inverse(inv, mats, lead, tag, "mi32_inv_det_device", want_inverse)
        assert st.tolist() == [OK] * batch, tag
        assert_pair(mant, exp, want_m, want_e, tag)
        if want_inverse:
            assert_members(oracle, x, st, pivoting, dtype, n, "steps", None, tag)


@pytest.mark.parametrize("c", [pytest.param(c, id=f"{c.name}-{c.n}") for c in G.DET_ANY])
def test_inv_det_any(oracle, det_large_dll, inverters, c):
    """One member above order 128 through ``mi32_inv_det_any_device*`` on the route ``inv`` runs, with a carved pair,
    with the inverse and without."""
    inv, bw = inverters(c.algo, c.pivoting), None
    if c.reference == "mirror64":
        bw = inv.resolved_blocking_f64(c.n)
        assert bw > 0
    elif c.dtype == F64:
        assert inv.resolved_blocking_f64(c.n) > 0
    else:
        assert inv.resolved_algo(c.n, 1) == {"blocked32": g.ALGO_BLOCKED, "nopivot_blocked32": g.ALGO_BLOCKED,
                                             "sweep32": g.ALGO_SWEEP, "wide": g.ALGO_WIDE}[c.name]
    a = matrix(c.pivoting, c.dtype, c.n)
    _, mst, piv, swp = mirror_blocked64(det_large_dll, a, bw) if bw else mirror_steps(det_large_dll, a, c.pivoting)
    want_m, want_e = expected_pair(a, piv, swp, c.pivoting)
    assert mst == OK and np.isfinite(piv).all()
    for want_inverse in (True, False):
        tag = ("inv_det_any", c.name, c.n, want_inverse)
        x, st, mant, exp = guarded_inverse(inv, a[None], G.LEAD_ODD, tag, "mi32_inv_det_any_device", want_inverse)
        assert st.tolist() == [OK], tag
        assert_pair(mant, exp, want_m, want_e, tag)
        if want_inverse:
            assert_members(oracle, x, st, c.pivoting, c.dtype, c.n, c.reference, bw, tag)


# ---- a null status -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,algo,n", G.NULL_STATUS, ids=[f[0] for f in G.NULL_STATUS])
def test_null_status(oracle, inverters, family, algo, n):
    """``d_status = NULL`` in the C ABI, and ``status=None`` in Python: the carved status buffer that was not passed keeps
    every bit, and so does everything around the output."""
    inv = inverters(algo, True)
    assert inv.resolved_algo(n, 2) == {"one_launch": g.ALGO_RESIDENT, "sweep": g.ALGO_SWEEP, "blocked": g.ALGO_BLOCKED}[family]
    ref = "through" if family == "blocked" else "steps"
    mats = batch_of(True, F32, n, 2)
    tag = ("null status", family, n)
    x, st, _, _ = guarded_inverse(inv, mats, G.LEAD_ODD, tag, "mi32_inv_device", null_status=True)
    assert st is None
    assert_members(oracle, x, None, True, F32, n, ref, None, tag)
    a, out = inputs(mats, G.LEAD_ODD), outputs(mats.shape, F32, G.LEAD_ODD)
    x, st = inv.inv(a.view, out=out.view)
    torch.cuda.synchronize()
    assert st.shape == (2,) and st.dtype == torch.int32 and st.tolist() == [OK, OK]
    a.assert_unchanged((tag, "a"))
    assert_members(oracle, out.assert_margins((tag, "out")), None, True, F32, n, ref, None, tag)


# ---- A X = B -------------------------------------------------------------------------------------------------------------
def guarded_solve(inv, mats, b, lead, in_place, tag):
    n = mats.shape[1]
    cols = b.shape[2] if b.ndim == 3 else 1
    a = inputs(mats, lead)
    rh = Guarded(b.shape, b.dtype, lead, G.NAN_IN[b.dtype.type], G.margin_for(n, cols), b)
    out = rh if in_place else Guarded(b.shape, b.dtype, lead, G.SENTINEL[b.dtype.type], G.margin_for(n, cols))
    st = words(mats.shape[0], I32, lead)
    x, s = inv.solve(a.view, rh.view, out=out.view, status=st.view)
    torch.cuda.synchronize()
    assert x.data_ptr() == out.view.data_ptr() and x.shape == b.shape and s.data_ptr() == st.view.data_ptr()
    a.assert_unchanged((tag, "a"))
    if not in_place:
        rh.assert_unchanged((tag, "b"))
    return out.assert_margins((tag, "x")), st.assert_margins((tag, "status"))


@pytest.mark.parametrize("dtype", [F32, F64], ids=dt_id)
@pytest.mark.parametrize("n", G.SOLVE_ORDERS)
def test_solve(solve_dll, inverters, n, dtype):
    """Two systems; K = 1, 3 and one column more than a launch holds, each into a separate ``out`` and in place; the
    vector form of ``b`` once.  The aligned control at K = 3."""
    inv, es = inverters("auto", True), np.dtype(dtype).itemsize
    mats = batch_of(True, dtype, n, 2)
    chunk = inv.resolved_solve(n, 1, es)[0]
    assert chunk == cap(n)
    for k in G.SOLVE_K + (chunk + 1,):
        launches = inv.resolved_solve(n, k, es)[1]
        assert launches == -(-k // chunk) and (k <= chunk or launches >= 2)
        b = np.stack([rhs(n, k, 8200 + 31 * n + m, dtype) for m in range(2)])
        want, want_st = mirror_solve_batch(solve_dll, mats, b)
        assert want_st.tolist() == [OK, OK] and np.isfinite(want).all()
        for lead in LEADS if k == 3 else LEADS[:1]:
            for in_place in (False, True):
                tag = ("solve", dt_id(dtype), n, k, lead, "in place" if in_place else "out")
                x, st = guarded_solve(inv, mats, b, lead, in_place, tag)
                assert st.tolist() == [OK, OK], tag
                assert G.same_bits(x, want), (tag, G.first_difference(x, want))
    b = np.stack([rhs(n, 1, 8200 + 31 * n + m, dtype) for m in range(2)])
    want, _ = mirror_solve_batch(solve_dll, mats, b)
    tag = ("solve", dt_id(dtype), n, "vectors")
    x, st = guarded_solve(inv, mats, b[:, :, 0], G.LEAD_ODD, False, tag)
    assert x.shape == (2, n) and st.tolist() == [OK, OK] and G.same_bits(x, want[:, :, 0]), tag


# ---- the residual verifier -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", G.RESIDUAL_ORDERS)
def test_residual(inverters, n):
    """``a`` and ``x`` carved: the three numbers of every member equal those of the call on tensors that start an
    allocation, bit for bit (so no NaN of a margin was read), and both inputs are unchanged.  The operands are
    ``residual_cases.integer_batch``: every partial sum is an exact integer, so the order of the kernel's atomics cannot
    show in the bits, and the two norms are also held to the int64 answer."""
    inv = inverters("auto", True)
    a, x = residual_cases.integer_batch(n, 2, 6100)
    plain = inv.residual(torch.from_numpy(a).cuda(), torch.from_numpy(x).cuda()).cpu().numpy()
    assert plain.shape == (2, 3) and np.isfinite(plain).all()
    assert G.same_bits(plain[:, :2], residual_cases.expected_exact(a, x)[:, :2])
    for lead in LEADS:
        ga, gx = inputs(a, lead), inputs(x, lead)
        r = inv.residual(ga.view, gx.view).cpu().numpy()
        assert G.same_bits(r, plain), (n, lead, r, plain)
        ga.assert_unchanged(("residual", n, lead, "a"))
        gx.assert_unchanged(("residual", n, lead, "x"))


# ---- views ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo,n", [("workgroup", 33), ("blocked", 130)], ids=["one_launch", "blocked"])
@pytest.mark.parametrize("view", ["transposed", "every_other", "expanded"])
def test_views(oracle, inverters, view, algo, n):
    """``inv`` of a view that is not contiguous equals ``inv`` of its contiguous copy bit for bit -- which is the
    reference's result -- and leaves the buffer the view was taken from unchanged."""
    inv = inverters(algo, True)
    ref = "through" if algo == "blocked" else "steps"
    src = inputs(batch_of(True, F32, n, 4), G.LEAD_ODD)
    v = {"transposed": src.view.transpose(1, 2), "every_other": src.view[::2],
         "expanded": src.view[1].expand(3, n, n)}[view]
    assert not v.is_contiguous()
    assert inv.resolved_algo(n, v.shape[0]) == (g.ALGO_BLOCKED if algo == "blocked" else g.ALGO_RESIDENT)
    x, st = inv.inv(v)
    copy = v.contiguous()
    x2, st2 = inv.inv(copy)
    torch.cuda.synchronize()
    assert st.tolist() == st2.tolist() == [OK] * v.shape[0]
    x, x2 = x.cpu().numpy(), x2.cpu().numpy()
    assert G.same_bits(x, x2), (view, G.first_difference(x, x2))
    src.assert_unchanged(("view", view, algo))
    if view == "every_other":
        assert_members(oracle, x, None, True, F32, n, ref, None, view, index=[0, 2])
    elif view == "expanded":
        assert_members(oracle, x, None, True, F32, n, ref, None, view, index=[1, 1, 1])
    else:
        for b in range(4):
            t = np.ascontiguousarray(matrix(True, F32, n, b).T)
            want = oracle.matrix_inv_32_inplace(t, n, zeros="through" if algo == "blocked" else "skip").reshape(n, n)
            assert G.same_bits(x[b], want), (view, b)


# ---- the refusals, through a live Inverter -------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(oracle, inverters):
    """Every refusal of tests/test_dense_args.py once through ``Inverter.inv`` / ``inv_det`` / ``solve``: ValueError, and
    the next valid call on the same handle gives the oracle's bits."""
    inv, n, batch = inverters("workgroup", True), 9, 3
    mats = batch_of(True, F32, n, batch)
    a = torch.from_numpy(mats).cuda()
    b = torch.from_numpy(np.stack([rhs(n, 2, 8300 + m) for m in range(batch)])).cuda()
    size = batch * n * n
    buf = torch.zeros(2 * size, device="cuda")
    buf[:size] = a.reshape(-1)
    inside = buf[:size].view(batch, n, n)
    bbuf = torch.zeros(2 * b.numel(), device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    dev = dict(device="cuda")
    refusals = {
        "a on the host": lambda: inv.inv(a.cpu()),
        "a on meta": lambda: inv.inv(torch.empty(batch, n, n, device="meta")),
        "out of another dtype": lambda: inv.inv(a, out=torch.empty(size // 2 + 1, dtype=torch.float64, **dev)),
        "out on the host": lambda: inv.inv(a, out=torch.empty(batch, n, n)),
        "out too short": lambda: inv.inv(a, out=torch.empty(size - 1, **dev)),
        "out too long": lambda: inv.inv(a, out=torch.empty(size + 1, **dev)),
        "out not contiguous": lambda: inv.inv(a, out=torch.empty(batch, n, n, **dev).transpose(1, 2)),
        "out is a": lambda: inv.inv(a, out=a),
        "out one element into a": lambda: inv.inv(inside, out=buf[1:size + 1]),
        "out ends in a": lambda: inv.inv(buf[size:].view(batch, n, n), out=buf[1:size + 1]),
        "status int64": lambda: inv.inv(a, status=torch.empty(batch, dtype=torch.int64, **dev)),
        "status on the host": lambda: inv.inv(a, status=torch.empty(batch, dtype=torch.int32)),
        "status short": lambda: inv.inv(a, status=torch.empty(batch - 1, **i32)),
        "status long": lambda: inv.inv(a, status=torch.empty(batch + 1, **i32)),
        "status strided": lambda: inv.inv(a, status=torch.empty(2 * batch, **i32)[::2]),
        "status 2-D": lambda: inv.inv(a, status=torch.empty(batch, 1, **i32)),
        "inv_det: out of another dtype": lambda: inv.inv_det(a, out=torch.empty(batch, n, n, dtype=torch.float64, **dev)),
        "inv_det: status short": lambda: inv.inv_det(a, status=torch.empty(1, **i32), want_inverse=False),
        "inv_det_any: status on the host": lambda: inv.inv_det_any(a, status=torch.empty(batch, dtype=torch.int32)),
        "solve: a on the host": lambda: inv.solve(a.cpu(), b.cpu()),
        "solve: out of another dtype": lambda: inv.solve(a, b, out=torch.empty(b.shape, dtype=torch.float64, **dev)),
        "solve: out on the host": lambda: inv.solve(a, b, out=torch.empty(b.shape)),
        "solve: out in a": lambda: inv.solve(inside, b, out=buf[3:3 + b.numel()].view(b.shape)),
        "solve: out partly over b": lambda: inv.solve(a, bbuf[:b.numel()].view(b.shape),
                                                      out=bbuf[1:b.numel() + 1].view(b.shape)),
        "solve: status short": lambda: inv.solve(a, b, status=torch.empty(batch - 1, **i32)),
        "solve: status on the host": lambda: inv.solve(a, b, status=torch.empty(batch, dtype=torch.int32)),
    }
    for name, call in refusals.items():
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"{name}: accepted")
        x, st = inv.inv(a)
        torch.cuda.synchronize()
        assert_members(oracle, x.cpu().numpy(), st.cpu().numpy(), True, F32, n, "steps", None, ("after", name))
    assert torch.equal(a.cpu(), torch.from_numpy(mats)) and torch.equal(buf[:size].cpu(), torch.from_numpy(mats).reshape(-1))
