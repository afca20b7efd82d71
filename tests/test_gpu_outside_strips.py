"""GPU tests of the strip(t) tiles of the columns outside a block (ostrip_body, mi32_update_tile.h): the block's earlier
steps as one matrix-core accumulation chain per element, then the sub-panel's own W steps (run with ``-m gpu`` on an
MI355X).

Every result is compared with the step-by-step CPU oracle byte for byte, -0.0 stored as +0.0 (``canon``); there is no
tolerance in this file.  Every input is asserted to have status 0 in the oracle.  The tiles ride in the panel launches
only for a single matrix or a small batch of more than one block: every test asserts that through ``resolved_route``
(``part_strips_at_end == 0``), so a plan that moved the strips to the block's end fails here instead of passing on
other code.

The shapes are the smallest that reach the tiles' edges: 640 rows at the default plan are blocks of 256 / 256 / 128
(the middle block has outside columns on both sides, K = c0 - C0 reaches 240 = 7.5 register chunks of 32 steps, the last
block is 128 wide); 600 rows put 40 padded rows first; block_width 128 with sub-panels of 4, 8 and 32 columns gives K
that is no multiple of the chunk, at most one chunk, and K = W.
"""
import numpy as np
import pytest

from degenerate_cases import block_diagonal, canon, signed_pow2_permutation
from resident_cases import dist_matrix, dominant, run

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_matrix_inversion_amd as g  # noqa: E402

OK = 0
_WANT = {}


def want_of(oracle, key, a, pivoting=True):
    """The step-by-step oracle's inverse (n, n) of ``a``, status asserted 0; computed once per key, left unchanged."""
    if key not in _WANT:
        n = a.shape[0]
        fn = oracle.matrix_inv_32_inplace if pivoting else oracle.matrix_inversion_no_pivots
        x, info = fn(a, n, return_info=True)
        assert int(info["status"]) == OK, key
        x = x.reshape(n, n)
        x.setflags(write=False)
        _WANT[key] = x
    return _WANT[key]


def dense(kind, n):
    return dist_matrix(kind, n, 9100 + n)


def first_difference(got, want):
    bad = np.argwhere(np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32))
    return None if not len(bad) else {"differing": len(bad), "first": tuple(int(v) for v in bad[0])}


def assert_rides(inv, n, batch, blocks):
    """More than one block, and the strip(t) tiles ride in the panel launches."""
    route, _ = inv.resolved_route(n, batch)
    assert route["nblocks"] == blocks > 1 and route["parts"] == 1 and route["part_strips_at_end"][0] == 0, route
    assert batch * -(-route["np"] // 64) <= 256 and route["np"] <= 4096


def check(inv, a, want, tag):
    got, st = run(inv, a)
    assert st.tolist() == [OK], (tag, st)
    assert got.dtype == np.float32 and canon(got) == canon(want), (tag, first_difference(got.reshape(want.shape), want))
    return got


@pytest.fixture(scope="module")
def inv_blocked():
    inv = g.Inverter(algo="blocked")
    yield inv
    inv.close()


@pytest.mark.parametrize("kind", ["gate", "ref100", "rand"])
@pytest.mark.parametrize("n", [640, 600])
def test_default_plan_three_blocks(oracle, inv_blocked, n, kind):
    """W 16, blocks 256 / 256 / 128: K up to 240; n = 600 pads 40 rows in front."""
    assert inv_blocked.resolved_blocking(n, 1) == (16, 256) and inv_blocked.resolved_panel_widths(n, 1) == [16, 16, 16]
    assert_rides(inv_blocked, n, 1, 3)
    assert inv_blocked.resolved_route(n, 1)[0]["np"] == 640
    a = dense(kind, n)
    check(inv_blocked, a, want_of(oracle, (kind, n), a), (kind, n))


@pytest.mark.parametrize("w", [4, 8, 32])
def test_narrow_blocks_every_panel_width(oracle, w):
    """block_width 128: K = W ... 128 - W in steps of W -- partial chunks (W 4, 8), one chunk or less, K = W."""
    n = 640
    inv = g.Inverter(algo="blocked", panel_width=w, block_width=128)
    try:
        assert inv.resolved_blocking(n, 1) == (w, 128) and inv.resolved_panel_widths(n, 1) == [w] * 5
        assert_rides(inv, n, 1, 5)
        for kind in ("gate", "ref100"):
            a = dense(kind, n)
            check(inv, a, want_of(oracle, (kind, n), a), (kind, w))
    finally:
        inv.close()


def test_no_pivot_strips_ride_the_diagonal_panels(oracle):
    n = 640
    inv = g.Inverter(algo="blocked", pivoting=False)
    try:
        assert inv.resolved_algo(n, 1) == g.ALGO_BLOCKED
        assert_rides(inv, n, 1, inv.resolved_route(n, 1)[0]["nblocks"])
        a = dominant(n, 9200, np.float32)
        check(inv, a, want_of(oracle, ("dominant", n), a, pivoting=False), "no pivot")
    finally:
        inv.close()


def test_batch_of_three_members(oracle, inv_blocked):
    """Three different members: the tiles' batch index; 18 and 24 tiles, so the four-group workgroups of the 1024-thread
    panel launches end with groups past the last tile.  Against the oracle and against three single calls."""
    n = 640
    assert_rides(inv_blocked, n, 3, 3)
    mats = np.stack([dense(kind, n) for kind in ("gate", "ref100", "rand")])
    want = [want_of(oracle, (kind, n), mats[b]) for b, kind in enumerate(("gate", "ref100", "rand"))]
    got, st = run(inv_blocked, mats)
    assert st.tolist() == [OK] * 3
    for b in range(3):
        assert canon(got[b]) == canon(want[b]), (b, first_difference(got[b], want[b]))
        single, st1 = run(inv_blocked, mats[b])
        assert st1.tolist() == [OK] and single.tobytes() == got[b].tobytes(), b


@pytest.mark.parametrize("family", ["block-diagonal", "permutation"])
def test_exact_zero_multipliers_are_multiplied_through(oracle, inv_blocked, family):
    """Most multipliers of the block's earlier steps are exact zeros (and most u_m too): the chain multiplies them
    through.  The inverse is known in closed form (permutation) or block by block; the oracle agrees with both."""
    n = 320
    if family == "block-diagonal":
        a, blocks = block_diagonal([100, 60, 90, 70], 9300)
    else:
        a, exact = signed_pow2_permutation(n, 9301)
    assert a.shape == (n, n)
    assert_rides(inv_blocked, n, 1, 2)
    want = want_of(oracle, (family, n), a)
    if family == "permutation":
        assert canon(want) == canon(exact)
    else:
        off, outside = 0, np.ones((n, n), bool)
        for blk in blocks:
            k = blk.shape[0]
            assert canon(want[off:off + k, off:off + k]) == canon(want_of(oracle, (family, "block", off), blk))
            outside[off:off + k, off:off + k] = False
            off += k
        assert not want[outside].any()
    check(inv_blocked, a, want, family)
