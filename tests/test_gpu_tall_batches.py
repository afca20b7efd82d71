"""Batches of the blocked fp32 path above 4096 padded rows, and the one-workgroup panels of 8 and 16 rows per lane
(run with ``-m gpu`` on an MI355X).  Each test first asserts the plan that routes it to the branch it is meant for
("Routing above 4096 rows"; tests/test_tall_batch_cases.py pins the same plans without a device),
so a change of the thresholds fails the test instead of emptying it.

Expected values come from the reference-order CPU oracle (two runs at N = 4200, shared by every test here), from its
committed digest at N = 8200, or from an exact transform of one of those (tests/tall_batch_cases.py); the split /
unsplit comparison is an extra.  No tolerance anywhere: bytes (-0.0 stored as +0.0) and literal status words.  A
flagged member's values are unspecified and never looked at."""
import numpy as np
import pytest

import tall_batch_cases as C
from conftest import canonical_bytes, check_against_oracle_digest, gate_matrix, load_oracle_digest
from degenerate_cases import zero_column

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_matrix_inversion_amd as g  # noqa: E402
from gpu_matrix_inversion_amd import _lib  # noqa: E402

N = C.N_TALL
ALL_16 = [16] * 17


@pytest.fixture
def inv_blocked():
    inv = g.Inverter(algo="blocked")
    yield inv
    inv.close()


def run_batch(inv, matrices):
    """(inverse, status) of one call on the stacked matrices: the inverse stays on the device, the status comes back."""
    mats = torch.from_numpy(np.stack(matrices)).cuda()
    x, st = inv.inv(mats)
    torch.cuda.synchronize()
    return x, st.tolist()


def assert_member_bits(oracle, x, b, member):
    want = C.expected_inverse(oracle, member)
    what = "base" if member.transform is None else f"variant 2^{member.transform.k}"
    assert canonical_bytes(x[b].cpu().numpy()) == canonical_bytes(want), f"member {b} ({member.base[0]} {what})"


# ---- a. shared panels with a batch index -----------------------------------------------------------------------------
@pytest.mark.parametrize("batch,rotate", [(2, 0), (2, 1), (3, 0), (4, 0)], ids=["2", "2-variant", "3", "4"])
def test_shared_panels_with_a_batch_index_bit_identical_to_oracle(oracle, inv_blocked, batch, rotate):
    """N = 4200, two workgroups per panel and member: gj_panel_multi_kernel on batch x 2 workgroups, every member with
    exchange granules, tags and a guard of its own.  Batches of 2 and 3: the strips ride behind the panel workgroups
    of the same launch; batch 4 (eight panel workgroups, the most the plan allows): strips at the block's end.  One
    member of every batch but the first is a 2^40-scaled variant (full division in its strips, beside a member on the
    fast one), and a variant's winning rows sit in other workgroups than its base's at the same step."""
    assert inv_blocked.resolved_panel_widths(N, batch) == ALL_16 and inv_blocked.resolved_blocking(N, batch) == (16, 256)
    route, groups = inv_blocked.resolved_route(N, batch)
    assert route["shared_panels"] == 1 and route["parts"] == 1 and groups[:2] == [2, 1]
    assert (route["part_strips_at_end"][0] == 0) == (batch < 4)
    members = C.tall_batch(N, batch, rotate)
    x, st = run_batch(inv_blocked, [m.matrix for m in members])
    assert st == [0] * batch
    for b, m in enumerate(members):
        assert_member_bits(oracle, x, b, m)


# ---- b. / f. N = 8200 ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide():
    dig = load_oracle_digest(C.N_WIDE)
    return dig, gate_matrix(C.N_WIDE, int(dig["seed"]))


def test_three_workgroup_panels_in_a_batch_of_two_bit_identical_to_oracle_digest(inv_blocked, wide):
    """N = 8200 (8320 padded rows), batch 2: three workgroups per panel and member, going 3 -> 2 inside the first block
    and 2 -> 1 later, with two members in flight.  Member 0 against the oracle's committed digest; member 1 is its
    row-permuted, sign-flipped, 2^-9-scaled variant, compared on the device with the exact transform of member 0's
    result -- which the digest has just proved to be the oracle's."""
    dig, a = wide
    n = C.N_WIDE
    assert inv_blocked.resolved_panel_widths(n, 2) == [16] * 33
    route, groups = inv_blocked.resolved_route(n, 2)
    assert route["shared_panels"] == 1 and [groups[b] for b in (0, 1, 17)] == [3, 2, 1]
    a1, t = C.variant(a, 8200, -9)
    x, st = run_batch(inv_blocked, [a, a1])
    assert st == [0, 0]
    check_against_oracle_digest(x[0].cpu().numpy(), dig)
    d = torch.from_numpy(t.d).cuda()
    perm = torch.from_numpy(t.perm).cuda()
    want1 = (x[0] * d[:, None])[:, perm] / 2.0 ** t.k   # sign flip, column gather, division by 2^k: all exact
    assert want1.dtype == torch.float32 and torch.equal(x[1], want1)
    assert not torch.equal(x[1], x[0])


def test_sixteen_rows_per_lane_w4_panel_bit_identical_to_oracle_digest(monkeypatch, wide):
    """gj_subpanel_kernel<1024, 16, 4, false>: above 8192 rows with shared panels off, one workgroup holds 16 rows
    per lane and W = 4 columns.  Every batch of five or more at such an order runs it (tests/test_tall_batch_cases.py:
    the plan of (8200, 5) is this one); a single matrix with MI32_MULTI_PANEL=0 keeps the test small."""
    dig, a = wide
    n = C.N_WIDE
    monkeypatch.setenv("MI32_MULTI_PANEL", "0")
    inv = g.Inverter(algo="blocked")
    try:
        assert inv.resolved_panel_widths(n, 1) == [4] + [8] * 16 + [16] * 16
        assert inv.resolved_blocking(n, 1) == (16, 256)
        x, st = run_batch(inv, [a])
    finally:
        inv.close()
    assert st == [0]
    check_against_oracle_digest(x[0].cpu().numpy(), dig)


# ---- c. flagged members do not disturb their neighbours --------------------------------------------------------------
@pytest.mark.parametrize("flagged_at", [0, 1])
@pytest.mark.parametrize("k", [15, 16])
def test_a_singular_member_of_a_shared_panel_batch_leaves_its_neighbour_alone(oracle, inv_blocked, k, flagged_at):
    """A zero column at step 15 (the last of the first shared sub-panel) or 16 (the first of the second) in one member
    of a batch of two, in either place: status 2 for it, status 0 and the oracle's bits for the other."""
    assert inv_blocked.resolved_panel_widths(N, 2) == ALL_16
    valid = C.tall_batch(N, 2)[1]
    bad = zero_column(N, k, C.SEED_GATE, base=C.cached_base("gate", N, C.SEED_GATE))
    mats = [valid.matrix, valid.matrix]
    mats[flagged_at] = bad
    x, st = run_batch(inv_blocked, mats)
    want = [0, 0]
    want[flagged_at] = 2
    assert st == want
    assert_member_bits(oracle, x, 1 - flagged_at, valid)


# ---- d. a lost partner in a batch ------------------------------------------------------------------------------------
def test_a_lost_partner_poisons_its_own_member_only(oracle, inv_blocked):
    """mi32_debug_drop_panel_group(1) (host side only) leaves out the last panel workgroup of the grid: member 1's
    second group.  Member 1's first group gives the partner up after its bounded wait: MI32_RUNTIME_ERROR and a
    NaN-filled inverse for member 1 -- and status 0 and the oracle's bits for member 0, whose panels ran beside it in
    every one of those launches.  The next call on the same handle is healthy for both.  (The documented time-out
    path, run once.)"""
    assert inv_blocked.resolved_panel_widths(N, 2) == ALL_16 and inv_blocked.resolved_route(N, 2)[1][0] == 2
    members = C.tall_batch(N, 2)
    lib = _lib.load()
    lib.mi32_debug_drop_panel_group(1)
    try:
        x, st = run_batch(inv_blocked, [m.matrix for m in members])
    finally:
        lib.mi32_debug_drop_panel_group(0)
    assert st == [0, _lib.MI32_RUNTIME_ERROR] and _lib.MI32_RUNTIME_ERROR == 3
    assert bool(torch.isnan(x[1]).all())
    assert_member_bits(oracle, x, 0, members[0])
    x2, st2 = run_batch(inv_blocked, [m.matrix for m in members])
    assert st2 == [0, 0]
    for b, m in enumerate(members):
        assert_member_bits(oracle, x2, b, m)


# ---- e. batches too large for shared panels --------------------------------------------------------------------------
@pytest.mark.parametrize("batch,bw,singular", [(5, 256, ()), (8, 128, (3, 6))], ids=["5", "8"])
def test_batches_beyond_shared_panels_split_and_unsplit_bit_identical_to_oracle(oracle, inv_blocked, monkeypatch,
                                                                                 batch, bw, singular):
    """N = 4200 with five and eight members: no shared panels, one 1024-thread workgroup per member holds 8 rows per
    lane (W = 8) in the first block; the batch runs as two halves (3 + 2, 4 + 4) on two streams, both with the whole
    batch's plan, and once more on one stream.  Eight members: block width 128, and a singular member in each half."""
    widths = inv_blocked.resolved_panel_widths(N, batch)
    assert widths == [8] + [16] * (len(widths) - 1) and len(widths) == -(-4224 // bw)
    assert inv_blocked.resolved_blocking(N, batch) == (16, bw)
    route = inv_blocked.resolved_route(N, batch)[0]
    assert (route["shared_panels"], route["parts"], route["part_batch"]) == (0, 2, [(batch + 1) // 2, batch // 2])
    members = C.tall_batch(N, batch)
    mats = [m.matrix for m in members]
    for b in singular:
        mats[b] = np.ones((N, N), np.float32)
    if singular:   # one in each half
        assert min(singular) < (batch + 1) // 2 <= max(singular)
    x_split, st_split = run_batch(inv_blocked, mats)
    monkeypatch.setenv("MI32_BATCH_SPLIT", "0")   # read per call
    assert inv_blocked.resolved_route(N, batch)[0]["parts"] == 1
    x_one, st_one = run_batch(inv_blocked, mats)
    want = [2 if b in singular else 0 for b in range(batch)]
    assert st_split == want and st_one == want
    ok = [b for b in range(batch) if b not in singular]
    assert torch.equal(x_split[ok], x_one[ok])
    for b in ok:
        assert_member_bits(oracle, x_split, b, members[b])


# ---- g. fp32 no-pivot batch ------------------------------------------------------------------------------------------
def test_no_pivot_batch_above_4096_rows_bit_identical_to_oracle(oracle):
    """fp32 without pivoting, N = 4200, batch 2: the plan has the shared-panel flag set, which this variant -- no panel
    search, the 16 x 16 diagonal block is its whole panel -- must ignore, with a batch index in every launch.  Member 0
    against the oracle's no-pivot restatement, member 1 its diagonally scaled variant."""
    a = C.dominant(N, 4200)
    a1, t = C.variant_nopivot(a, 4201)
    inv = g.Inverter(algo="auto", pivoting=False)
    try:
        assert inv.resolved_algo(N, 2) == g.ALGO_BLOCKED
        assert inv.resolved_panel_widths(N, 2) == ALL_16   # the flag: what a pivoting plan with shared panels gets
        x, st = run_batch(inv, [a, a1])
    finally:
        inv.close()
    assert st == [0, 0]
    want = oracle.matrix_inversion_no_pivots(a, N)
    assert canonical_bytes(x[0].cpu().numpy()) == canonical_bytes(want)
    assert canonical_bytes(x[1].cpu().numpy()) == canonical_bytes(C.apply_variant_nopivot(want, t))


# ---- h. the route a live context reports ---------------------------------------------------------------------------
def test_a_context_routes_as_the_null_handle_does_until_its_second_stream_is_turned_off(inv_blocked):
    """mi32_resolve_route with a handle: a fresh context has both streams, as the null handle assumes
    (tests/test_tall_batch_cases.py pins those answers); mi32_set_lookahead(h, 0) takes the look-ahead and the split
    away.  No inversion runs."""
    assert inv_blocked.resolved_route(N, 2) == _lib.resolve_route(None, N, 2)
    assert inv_blocked.resolved_route(N, 1)[0]["lookahead"] == 1 and inv_blocked.resolved_route(N, 5)[0]["parts"] == 2
    inv_blocked.set_lookahead(False)
    assert inv_blocked.resolved_route(N, 1)[0]["lookahead"] == 0
    off = inv_blocked.resolved_route(N, 5)[0]
    assert (off["parts"], off["part_batch"]) == (1, [5, 0])
