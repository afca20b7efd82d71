"""CPU proof of tests/sequence_cases.py, before the GPU sees any of it: the library plans every step of
tests/test_gpu_sequences.py onto the route the step is meant for -- asked through the C ABI with a null handle, the plan
code needs no device -- and the CPU oracle gives every step's inputs the status the step expects.  Literal plan values;
no tolerance."""
import numpy as np
import pytest

import sequence_cases as S
from conftest import canonical_bytes

from gpu_matrix_inversion_amd import _lib

KNOBS = ("MI32_PANEL_W", "MI32_BLOCK_W", "MI32_BLOCK_W64", "MI32_MULTI_PANEL", "MI32_ALGO", "MI32_LOOKAHEAD_MIN",
         "MI32_BATCH_SPLIT", "MI32_LOOKAHEAD")


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)


def route(n, batch=1):
    return _lib.resolve_route(None, n, batch)[0]


def test_the_split_batch_runs_as_33_and_32_members_at_block_width_128():
    assert S.SPLIT_BATCH * S.SPLIT_N ** 2 >= 64 * 1024 * 1024
    r = route(S.SPLIT_N, S.SPLIT_BATCH)
    assert (r["parts"], r["part_batch"], r["block_width"], r["shared_panels"], r["lookahead"]) == (2, [33, 32], 128, 0, 0)
    first = S.SPLIT_BATCH - S.SPLIT_BATCH // 2
    assert first == 33 and S.SPLIT_SINGULAR[0] < first <= S.SPLIT_SINGULAR[1]          # a singular member in either half
    assert S.SPLIT_ORACLE_MEMBERS == (0, first - 1, first, S.SPLIT_BATCH - 1)            # both ends of either half
    # one member fewer is below 64 Mi elements: no split, block width 256
    assert (route(S.SPLIT_N, 63)["parts"], route(S.SPLIT_N, 63)["block_width"]) == (1, 256)


def test_the_lookahead_step_needs_its_knob_and_the_tall_steps_do_not(monkeypatch):
    assert (route(2048)["np"], route(2048)["lookahead"]) == (2048, 0)
    (name, value), = S.LOOKAHEAD_ENV.items()
    monkeypatch.setenv(name, value)
    assert route(2048)["lookahead"] == 1 and route(2048)["shared_panels"] == 0 and route(1920)["lookahead"] == 0
    assert route(130)["lookahead"] == 0
    monkeypatch.delenv(name)
    tall = route(S.N_TALL)
    assert (tall["np"], tall["shared_panels"], tall["lookahead"], tall["parts"]) == (4224, 1, 1, 1)
    pair = route(S.N_TALL, 2)
    assert (pair["shared_panels"], pair["lookahead"], pair["parts"]) == (1, 0, 1)


def test_130_rows_are_one_outer_block_and_300_are_two():
    assert (route(130)["np"], route(130)["nblocks"]) == (256, 1)
    assert (route(300)["np"], route(300)["nblocks"]) == (384, 2)
    assert (route(200)["np"], route(200)["nblocks"]) == (256, 1)
    assert (route(160, 3)["nblocks"], route(160, 3)["parts"]) == (1, 1)
    assert (route(600)["np"], route(600)["nblocks"]) == (640, 3)


@pytest.mark.parametrize("name", sorted(S.ROUTE_FACTS))
def test_route_facts_the_gpu_tests_assert_on_their_live_handles(monkeypatch, name):
    """The same table, asked of a null handle under the step's own environment."""
    step = S.BY_NAME[name]
    for key, value in step.env.items():
        monkeypatch.setenv(key, value)
    r = route(step.n, step.batch)
    facts = S.ROUTE_FACTS[name]
    assert {k: r[k] for k in facts} == facts


def _resolved_f64(n):
    return S.block_width_f64(n)


@pytest.mark.parametrize("step", S.S1 + S.S2 + list(S.EXTRA.values()), ids=lambda s: s.name)
def test_every_step_resolves_to_the_algorithm_its_row_claims(monkeypatch, step):
    """With a null handle: AUTO and pivoting, what a fresh context does.  A step that sets the sweep on the live handle
    is asked with MI32_ALGO, which mi32_set_algo overrides and plan code reads in the same place; a no-pivot step's
    cross-over (512) lies below its order, so the pivoting answer is its answer too (the GPU test asks the live handle)."""
    lib = _lib.load()
    if step.algo != S.ALGO_AUTO:
        monkeypatch.setenv("MI32_ALGO", str(step.algo))
    if step.dtype == np.float32:
        assert lib.mi32_resolve_algo(None, step.n, step.batch) == step.resolves
        assert lib.mi32_workspace_bytes(step.n, step.batch, step.algo) > 0
    elif step.route == "blocked64":
        assert _resolved_f64(step.n) in (64, 128, 256) and _resolved_f64(255) == 0
    elif step.route == "sweep64":
        assert _resolved_f64(step.n) == 0
    else:
        assert step.route == "nopivot64" and not step.pivoting and step.n >= 512
    if not step.pivoting:
        assert step.n >= 512
    assert (S.ALGO_AUTO, S.ALGO_SWEEP, S.ALGO_BLOCKED) == (_lib.ALGO_AUTO, _lib.ALGO_SWEEP, _lib.ALGO_BLOCKED)


def test_neighbouring_steps_of_s1_are_of_different_kinds_and_the_workspace_grows_on_the_way():
    kinds = [(s.route, s.n, s.batch) for s in S.S1]
    # (the last step repeats 3b's call behind step 8's, which has its shape: the same carve over another matrix's data)
    assert all(a != b for a, b in zip(kinds[:-1], kinds[1:-1])) and kinds[-1] == kinds[-2] == kinds[3]
    assert {s.route for s in S.S1} == {"blocked32", "nopivot32", "sweep32", "sweep64", "blocked64", "nopivot64", "residual"}
    ws = _lib.load().mi32_workspace_bytes
    # fp32 blocked: a later, larger order needs more than every fp32 step before it
    assert ws(130, 1, 0) <= ws(200, 1, 0) < ws(300, 1, 0) < ws(160, 3, 0) < ws(600, 1, 0)
    assert ws(130, 1, 0) < ws(2048, 1, 0) < ws(S.N_TALL, 1, 0) < ws(S.N_TALL, 2, 0)
    assert ws(20, 1, 0) < ws(300, 1, S.ALGO_SWEEP)


@pytest.mark.parametrize("step", [s for s in S.S1 + list(S.EXTRA.values()) if s.route != "residual"] + [S.S2[1], S.S2[2]],
                         ids=lambda s: s.name)
def test_the_oracle_gives_every_step_the_status_it_expects(oracle, step):
    """(The three N = 4200 steps are left to the GPU module: their one oracle run takes seconds, and
    tests/test_tall_batch_cases.py proves the transform they rest on.)"""
    a = S.members(step)
    assert a.shape == (step.batch, step.n, step.n) and a.dtype == step.dtype
    xs, sts = S.expected(oracle, step)
    assert sts == step.status and all(st in (S.STATUS_OK, S.STATUS_SINGULAR) for st in sts)
    for x, st in zip(xs, sts):
        assert (x is None) == (st != S.STATUS_OK)
        if x is not None:
            assert x.shape == (step.n, step.n) and x.dtype == step.dtype and np.isfinite(x).all()
    if step.route in ("nopivot64", "blocked64", "sweep32", "sweep64"):
        # np.array_equal tells -0.0 from nothing, but no entry of these dense inverses is a zero of either sign
        assert all((x != 0).all() for x in xs if x is not None)


def test_the_steps_that_share_an_input_and_those_that_must_not():
    by = S.BY_NAME
    assert S.inputs(by["9"]) is S.inputs(by["3b"])
    assert not np.array_equal(S.inputs(by["8"]), S.inputs(by["3b"]))
    small = [S.inputs(by[k]).tobytes() for k in ("3a", "small-130", "c-130-a", "c-130-b", "c-130-c")]
    assert len(set(small)) == len(small)
    assert np.isnan(S.inputs(by["2"])).sum() == 1
    assert (S.inputs(by["6"])[1] == 1).all()
    spd = S.inputs(by["7a"])
    assert spd.dtype == np.float32 and S.inputs(by["7b"]).dtype == np.float64
    assert np.array_equal(spd, S.inputs(by["7b"]).astype(np.float32))
    import nopivot_cases
    assert nopivot_cases.dominant_share(spd) == 0.0


def test_split_members_are_exact_variants_of_the_four_oracle_members(oracle):
    """One variant member against the oracle itself: the transform, not the oracle, gives the other 58 their expected
    inverses."""
    step = S.SPLIT
    ms = S.split_members()
    xs, sts = S.expected(oracle, step)
    assert [b for b, st in enumerate(sts) if st != S.STATUS_OK] == list(S.SPLIT_SINGULAR)
    assert all(ms[b].transform is None for b in S.SPLIT_ORACLE_MEMBERS + S.SPLIT_SINGULAR)
    others = [b for b in range(S.SPLIT_BATCH) if b not in S.SPLIT_ORACLE_MEMBERS + S.SPLIT_SINGULAR]
    assert all(ms[b].transform is not None for b in others)
    assert len({ms[b].matrix.tobytes() for b in range(S.SPLIT_BATCH)}) == S.SPLIT_BATCH
    b = 38   # a 2^40 variant: base 2
    assert ms[b].transform.k == 40 and ms[b].base == 2
    x, info = oracle.matrix_inv_32_inplace(ms[b].matrix, step.n, return_info=True)
    assert info["status"] == 0 and canonical_bytes(x) == canonical_bytes(xs[b])
    assert canonical_bytes(xs[b]) != canonical_bytes(xs[S.SPLIT_ORACLE_MEMBERS[2]])


def test_same_compares_bytes_and_dtype():
    step = S.BY_NAME["3a"]
    x = np.arange(4, dtype=np.float32).reshape(2, 2)
    y = x.copy()
    y[0, 0] = -0.0
    assert S.same(step, y, x) and not S.same(step, x.astype(np.float64), x)
    y[1, 1] = np.nextafter(np.float32(3), np.float32(4))
    assert not S.same(step, y, x)
    sweep = S.BY_NAME["4a"]
    z = x.copy()
    assert S.same(sweep, z, x)
    z[1, 0] = np.nextafter(np.float32(2), np.float32(3))
    assert not S.same(sweep, z, x)
    z = x.copy()
    z[0, 0] = -0.0
    assert S.same(sweep, z, x)   # np.array_equal: the routes compared with it have no zero in their results (above)
