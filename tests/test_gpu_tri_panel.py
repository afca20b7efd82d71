"""GPU checks of the triangular panel steps (mi32_panel.h; panel_tri, mi32_internal.h) and of the update tiles that
rebuild G_s from multipliers and pivot rows.  Every panel instance of the blocked fp32 path, reached at the smallest
order that reaches it, gives the oracle's bits and status; the degenerate inputs run both at n = 300 (full steps) and
at n = 3100, where the first panels are the triangular instance.  Which instance a panel is comes from the library
itself (mi32_debug_panel_instance: what blocked_invert derives from the route), never from a copy of its rules."""
import ctypes

import numpy as np
import pytest

from conftest import gate_matrix
from degenerate_cases import canon, signed_pow2_permutation, zero_column, zero_row
from panel_tie_cases import oracle_inverse, tie_matrix

pytestmark = pytest.mark.gpu

TRI_INSTANCE = (1024, 4, 16, 0, 1)  # threads, rows per lane, columns, fused, workgroups: the one with triangular steps
N_TRI = 3100                        # smallest order of the table below whose first panels are that instance

# order -> (padded order, sub-panel s of block 0, (threads, rows per lane, columns, fused, workgroups), triangular):
# what the plan gives the first panels (below 2048 rows it runs them on 512 threads; the 1024-thread instances with
# one and two rows per lane are reached by the later blocks of n = 2100, see REQUIRED)
INSTANCES = {
    200: (256, 0, (256, 1, 16, 0, 1), 0), 400: (512, 0, (512, 1, 16, 0, 1), 0), 900: (1024, 0, (512, 2, 16, 0, 1), 0),
    1100: (1152, 1, (512, 4, 16, 1, 1), 0), 2100: (2176, 0, (1024, 3, 16, 0, 1), 0),
    3100: (3200, 0, TRI_INSTANCE, 1),
}
# the instances C1 runs: every one of them must be reached by the orders above
REQUIRED = {(256, 1, 16, 1, 1), (512, 1, 16, 1, 1), (1024, 1, 16, 1, 1), (1024, 2, 16, 1, 1), (1024, 2, 16, 0, 1),
            (1024, 3, 16, 0, 1), TRI_INSTANCE}


def instance(inv, n, batch, blk, s):
    """(threads, rows per lane, columns, fused, workgroups per panel, triangular) of panel s of block blk."""
    from gpu_matrix_inversion_amd import _lib

    out = (ctypes.c_int * 6)()
    fn = _lib.load().mi32_debug_panel_instance
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    fn.restype = ctypes.c_int
    assert fn(inv._h, n, batch, blk, s, out) == 0
    return tuple(out)


def instances_of(inv, n, batch=1):
    """Every instance the panels of this shape run."""
    route, _groups = inv.resolved_route(n, batch)
    widths = inv.resolved_panel_widths(n, batch)
    seen = set()
    for blk in range(route["nblocks"]):
        kb = min(route["block_width"], route["np"] - blk * route["block_width"])
        seen |= {instance(inv, n, batch, blk, s) for s in range(kb // widths[blk])}
    return seen


def run(inv, a):
    import torch

    x, st = inv.inv(torch.from_numpy(np.array(a)).cuda())  # (a copy: the shared references are read-only)
    torch.cuda.synchronize()
    return x.cpu().numpy(), st.cpu().numpy()


@pytest.fixture(scope="module")
def inv_blocked():
    import gpu_matrix_inversion_amd as g

    inv = g.Inverter(algo="blocked")
    yield inv
    inv.close()


_WANT = {}


def reference(oracle, name, n):
    """(input, oracle inverse, oracle status) of a named input at order n: computed once, left unchanged."""
    if (name, n) not in _WANT:
        rng = np.random.default_rng([9, n])
        a = {"gate": lambda: gate_matrix(n, 31_000 + n),
             "u100": lambda: rng.uniform(0, 100, (n, n)).astype(np.float32),
             "subnormal": lambda: (gate_matrix(n, 31_000 + n).astype(np.float64) * 2.0 ** -128).astype(np.float32),
             "ties": lambda: tie_matrix(n, (1, 8, 64), 77_000 + n)[0],
             "pow2": lambda: signed_pow2_permutation(n, 5)[0]}[name]()
        want, info = oracle_inverse(oracle, a, n)
        for v in (a, want):
            v.setflags(write=False)
        _WANT[name, n] = (a, want, info["status"])
    return _WANT[name, n]


@pytest.mark.parametrize("n", sorted(INSTANCES))
def test_every_instance_bit_identical_to_oracle(oracle, inv_blocked, n):
    np_, s, inst, tri = INSTANCES[n]
    assert inv_blocked.resolved_route(n)[0]["np"] == np_
    assert instance(inv_blocked, n, 1, 0, s) == inst + (tri,)  # the instance really is reached
    for name in ("gate", "u100"):
        a, want, status = reference(oracle, name, n)
        got, st = run(inv_blocked, a)
        assert st[0] == status, (name, st)
        assert canon(got) == canon(want), name


def test_only_the_measured_instance_is_triangular(inv_blocked):
    """Over every panel of C1 (and of a batch of 8 at 8192, whose panels hold 8 rows per lane): triangular steps on
    <1024,4,16,false> with one workgroup, nowhere else."""
    seen = set()
    for n, batch in ((4096, 1), (N_TRI, 4), (300, 1), (8192, 8)):
        seen |= instances_of(inv_blocked, n, batch)
    for inst in seen:
        assert inst[5] == (inst[:5] == TRI_INSTANCE), inst
    assert TRI_INSTANCE + (1,) in seen and len(seen) > 6
    # and the orders of test_every_instance_bit_identical_to_oracle reach every instance C1 runs
    reached = set().union(*(instances_of(inv_blocked, n) for n in INSTANCES))
    assert REQUIRED <= {inst[:5] for inst in reached}, REQUIRED - {inst[:5] for inst in reached}


@pytest.mark.parametrize("name", ["subnormal", "ties", "pow2"])
def test_degenerate_inputs_through_the_triangular_instance(oracle, inv_blocked, name):
    """gate * 2^-128 (the recursion's IEEE division on subnormal dividends and pivots), exact ties, exact powers of
    two with zero multipliers, at an order whose first 8 panels run triangular steps."""
    n = N_TRI
    assert instance(inv_blocked, n, 1, 0, 0)[5] == 1 and instance(inv_blocked, n, 1, 0, 7)[5] == 1
    a, want, status = reference(oracle, name, n)
    got, st = run(inv_blocked, a)
    assert st[0] == status == 0, name
    assert canon(got) == canon(want), name


def test_batch_with_a_singular_member_inside_a_triangular_panel(oracle, inv_blocked):
    """Member 2's column 21 is zero: its pivot is met in step 9 of sub-panel 7 of block 0, a triangular panel, whose
    recursion then divides by that zero pivot.  Status 2 for it; the neighbours keep the oracle's bits."""
    n, k = N_TRI, 21
    np_ = inv_blocked.resolved_route(n, 4)[0]["np"]
    s = (np_ - n + k) // 16  # the identity padding comes first
    assert instance(inv_blocked, n, 4, 0, s) == TRI_INSTANCE + (1,)
    gate, want_gate, _ = reference(oracle, "gate", n)
    u100, want_u100, _ = reference(oracle, "u100", n)
    mats = np.stack([gate, u100, zero_column(n, k, 0, base=gate), gate])
    got, st = run(inv_blocked, mats)
    assert list(st) == [0, 0, 2, 0]
    for b, want in ((0, want_gate), (1, want_u100), (3, want_gate)):
        assert canon(got[b]) == canon(want), b


# ---- the same inputs where every panel runs the full step ------------------------------------------------------------
@pytest.fixture(scope="module")
def a300():
    return gate_matrix(300, 31_300)


@pytest.mark.parametrize("pw", [8, 32])
def test_other_panel_widths(oracle, a300, pw):
    import gpu_matrix_inversion_amd as g

    inv = g.Inverter(algo="blocked", panel_width=pw, block_width=128)
    assert set(inv.resolved_panel_widths(300)) == {pw}
    got, st = run(inv, a300)
    inv.close()
    want, info = oracle.matrix_inv_32_inplace(a300, 300, return_info=True)
    assert st[0] == info["status"] == 0 and canon(got) == canon(want)


def test_batch_with_a_late_singular_member(oracle, inv_blocked, a300):
    n = 300
    mats = np.stack([a300, gate_matrix(n, 1), zero_row(n, 150, 2), gate_matrix(n, 3)])
    got, st = run(inv_blocked, mats)
    assert list(st) == [0, 0, 2, 0]
    for b in (0, 1, 3):
        assert canon(got[b]) == canon(oracle.matrix_inv_32_inplace(mats[b], n)), b


@pytest.mark.parametrize("name", ["subnormal", "ties", "pow2"])
def test_degenerate_inputs_through_full_steps(oracle, inv_blocked, name):
    a, want, status = reference(oracle, name, 300)
    got, st = run(inv_blocked, a)
    assert st[0] == status == 0, name
    assert canon(got) == canon(want), name


def test_panels_that_still_write_gt(oracle):
    """The no-pivot diagonal panel and the multi-workgroup panel keep the full step and their G_s store."""
    import gpu_matrix_inversion_amd as g

    n = 640
    a = (np.random.default_rng(12).uniform(-1, 1, (n, n)) + np.sqrt(n) * 4 * np.eye(n)).astype(np.float32)
    inv = g.Inverter(algo="blocked", pivoting=False)
    got, st = run(inv, a)
    inv.close()
    want, info = oracle.matrix_inversion_no_pivots(a, n, return_info=True)
    assert st[0] == info["status"] == 0 and canon(got) == canon(np.asarray(want, dtype=np.float32))
    n = 4200
    inv = g.Inverter(algo="blocked")
    assert instance(inv, n, 1, 0, 0)[4:] == (2, 0)  # two workgroups, full steps
    a, want, status = reference(oracle, "gate", n)
    got, st = run(inv, a)
    inv.close()
    assert st[0] == status == 0 and canon(got) == canon(want)
