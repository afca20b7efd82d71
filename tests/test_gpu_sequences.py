"""Back-to-back calls on one context (run with ``-m gpu`` on an MI355X): what the host layer promises of a call on a
live context, which no single-call test can see ("Ordering and workspace contract").

  A. one context serves every route from one workspace: sequences of calls of different routes, dtypes and shapes,
     enqueued without a host synchronisation in between, each over what the one before left in the workspace;
  B. a call is an ordinary citizen of its stream: enqueued while its input is still being produced, its output read
     and its input and output overwritten right behind it -- on a stream of torch's and on the default stream;
  C. the stream changes between calls while the earlier call is still running.

Each test first asserts, on the live handle, the route of every call it makes (tests/sequence_cases.py holds the
tables, tests/test_sequence_cases.py pins them without a device).  Expected values come from the CPU oracle of each
call's route, computed once per process: bytes (-0.0 stored as +0.0 on the blocked fp32 routes) and literal status
words, no tolerance but the residual's (that of test_device_residual_matches_oracle); a flagged member's values are
never looked at.  A comparison with a synchronous run of the same context is an extra where it appears.

The delay in front of a pending call is ``torch.cuda._sleep``, calibrated once per module with a pair of events to
DELAY_MS of GPU time; every test that relies on it asserts that the work was still pending when the library returned.
"""
import time

import numpy as np
import pytest

import sequence_cases as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_matrix_inversion_amd as g  # noqa: E402
from gpu_matrix_inversion_amd import _lib  # noqa: E402

DELAY_MS = 50.0
_DEVICE_INPUTS = {}


def device_input(step):
    """The step's input on the device: uploaded once per process and never written."""
    key = S.SAME_INPUT.get(step.name, step.name)
    if key not in _DEVICE_INPUTS:
        _DEVICE_INPUTS[key] = torch.from_numpy(np.array(S.inputs(step))).cuda()   # (a writable copy, for torch)
    return _DEVICE_INPUTS[key]


def garbage_like(a):
    return torch.full_like(a, float("nan"))


def garbage_status(step):
    return torch.full((step.batch,), -7, dtype=torch.int32, device="cuda")


def assert_route(inv, step):
    """The live handle, with the step's settings and environment in place, runs the step on the route it is meant for."""
    if step.dtype == np.float32:
        assert inv.resolved_algo(step.n, step.batch) == step.resolves, step.name
        if step.route in ("blocked32", "nopivot32"):
            route = inv.resolved_route(step.n, step.batch)[0]
            facts = S.ROUTE_FACTS.get(step.name, {})
            assert {k: route[k] for k in facts} == facts, (step.name, route)
    else:
        bw = inv.resolved_blocking_f64(step.n)
        assert (bw == 0) == (step.route == "sweep64"), (step.name, bw)
        if step.route == "blocked64":
            assert bw == S.block_width_f64(step.n)   # the width the oracle's mirror is run with


def enqueue(inv, monkeypatch, step, a, out, status):
    """One call of the step on torch's current stream: its settings on the live handle and its environment for this
    call only, the route asserted, nothing awaited."""
    lib = inv._lib
    with monkeypatch.context() as m:
        for name, value in step.env.items():
            m.setenv(name, value)
        _lib.check(lib.mi32_set_algo(inv._h, step.algo), "mi32_set_algo")
        _lib.check(lib.mi32_set_pivoting(inv._h, 1 if step.pivoting else 0), "mi32_set_pivoting")
        try:
            assert_route(inv, step)
            x, st = inv.inv(a, out=out, status=status)
        finally:
            _lib.check(lib.mi32_set_algo(inv._h, S.ALGO_AUTO), "mi32_set_algo")
            _lib.check(lib.mi32_set_pivoting(inv._h, 1), "mi32_set_pivoting")
    assert st is status and x.data_ptr() == out.data_ptr()


def check(oracle, step, out, status, tag):
    """Status words and, member by member, the oracle's inverse under the route's comparison."""
    xs, sts = S.expected(oracle, step)
    assert status.tolist() == sts == step.status, (tag, step.name)
    got = out.cpu().numpy().reshape(step.batch, step.n, step.n)
    for b, x in enumerate(xs):
        if x is not None:
            assert S.same(step, got[b], x), (tag, step.name, f"member {b}")


@pytest.fixture
def inv_auto():
    inv = g.Inverter(algo="auto")
    yield inv
    torch.cuda.synchronize()
    inv.close()


class Delay:
    def __init__(self, cycles, ms):
        self.cycles, self.ms = cycles, ms

    def enqueue(self):
        torch.cuda._sleep(self.cycles)


@pytest.fixture(scope="module")
def delay():
    """torch.cuda._sleep for about DELAY_MS of GPU time on the current stream: the cycle count is calibrated with a
    pair of events, then the delay itself is measured once."""
    def timed(cycles):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(cycles)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    torch.cuda.synchronize()
    timed(10_000)   # loads the kernel
    probe = 2_000_000
    ms = timed(probe)
    assert ms > 0.05, ms
    cycles = min(int(probe * DELAY_MS / ms), 1000 * probe)
    got = timed(cycles)
    print(f"\n[sequences] delay: torch.cuda._sleep({cycles}) = {got:.1f} ms of GPU time (probe {probe} cycles = {ms:.2f} ms)")
    assert 0.5 * DELAY_MS <= got <= 4 * DELAY_MS, got
    return Delay(cycles, got)


# ---- A. workspace history ---------------------------------------------------------------------------------------------
def run_sequence(oracle, inv, monkeypatch, groups, tag):
    """Every step of every group enqueued back to back on the current stream, each into tensors of its own; ONE
    synchronisation at the end, then every comparison."""
    steps = [s for grp in groups for s in grp]
    calls = [s for s in steps if s.route != "residual"]
    dev = {s.name: device_input(s) for s in steps}
    outs = {s.name: garbage_like(dev[s.name]) for s in calls}
    sts = {s.name: garbage_status(s) for s in calls}
    del_me = torch.empty(8, 3, dtype=torch.float64, device="cuda")   # the residual's output comes from the allocator's cache
    del del_me
    torch.cuda.synchronize()
    residuals = {}
    latest = {}   # input key -> name of the latest call enqueued on it
    t0 = time.perf_counter()
    for s in steps:
        key = S.SAME_INPUT.get(s.name, s.name)
        if s.route == "residual":   # on the pair (input, not yet computed output) of the latest call on that input
            assert inv.resolved_algo(s.n, 1) == S.ALGO_BLOCKED
            residuals[s.name] = inv.residual(dev[s.name], outs[latest[key]])
        else:
            enqueue(inv, monkeypatch, s, dev[s.name], outs[s.name], sts[s.name])
            latest[key] = s.name
    host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    print(f"\n[sequences] {tag}: {len(steps)} steps enqueued in {host_ms:.1f} ms of host time")
    for s in calls:
        check(oracle, s, outs[s.name], sts[s.name], tag)
    for name, r in residuals.items():
        step = S.BY_NAME[name]
        pair = S.BY_NAME[S.SAME_INPUT[name]]
        a = S.inputs(pair)
        want = S.expected_residual(oracle, a, S.expected(oracle, pair)[0][0])
        r = r.cpu().numpy()
        assert r.shape == (1, 3) and step.n == pair.n
        assert r[0, 0] == pytest.approx(want[0], rel=1e-9)
        assert r[0, 1] == pytest.approx(want[1], rel=1e-9)
        assert r[0, 2] == pytest.approx(want[2], rel=1e-6, abs=1e-12)
    return outs


def s1_groups():
    """S1 with the residual and the call behind it kept together: the unit a reversal moves."""
    groups, i = [], 0
    while i < len(S.S1):
        k = 2 if S.S1[i].route == "residual" else 1
        groups.append(S.S1[i:i + k])
        i += k
    return groups


@pytest.mark.parametrize("order", ["listed", "reversed"])
def test_s1_every_route_of_one_context_back_to_back_matches_the_oracle(oracle, inv_auto, monkeypatch, order):
    """fp64 blocked, fp32 blocked with a NaN (non-finite values stay behind), one and two outer blocks, both sweeps,
    a batch with a singular member, both no-pivot paths on an SPD input, the residual check (it memsets the head of the
    workspace) with a call right behind it, and the first two-block call again: on one context and one stream with no
    host synchronisation in between, so every carve lies over another route's data.  Listed: what the fp32 steps need
    grows along the list (tests/test_sequence_cases.py).  Reversed, on a fresh context: the largest come right after
    step 9, and the workspace is freed and allocated anew while calls that use it are enqueued."""
    groups = s1_groups()
    assert [s.name for grp in groups for s in grp] == [s.name for s in S.S1] and ["8r", "8"] in [[s.name for s in grp] for grp in groups]
    if order == "reversed":
        groups = groups[::-1]
        assert [s.name for s in groups[0]] == ["9"] and [s.name for s in groups[-1]] == ["1"]
    outs = run_sequence(oracle, inv_auto, monkeypatch, groups, f"S1 {order}")
    assert torch.equal(outs["9"], outs["3b"])   # the same call twice: the same bytes (and the oracle's, above)
    assert not torch.equal(outs["8"], outs["3b"])


def test_s2_tall_calls_share_one_workspace_with_lookahead_and_small_calls_between_them(oracle, inv_auto, monkeypatch):
    """N = 4200 (shared two-workgroup panels and the look-ahead), N = 2048 with the look-ahead forced, N = 130, the
    exact 2^40 variant of the first matrix, and the batch of the two: one context, nothing in between.  The last two
    follow a shared-panel call whose exchange tags started at 1 as well and whose row maps are still in the workspace:
    what the two memsets at the head of blocked_invert exist for."""
    run_sequence(oracle, inv_auto, monkeypatch, [[s] for s in S.S2], "S2")


# ---- B. behind a pending producer, in front of an eager consumer ------------------------------------------------------
B_CASES = ["3b", "4a", "la-2048", S.SPLIT.name, "1", "tall-base"]


def stream_of(kind):
    return torch.cuda.Stream() if kind == "fresh" else torch.cuda.default_stream()


@pytest.mark.parametrize("kind", ["fresh", "default"])
@pytest.mark.parametrize("name", B_CASES)
def test_a_call_behind_a_pending_producer_and_in_front_of_an_eager_consumer(oracle, monkeypatch, delay, name, kind):
    """On stream s: a delay, then the copy that produces the input, then the call -- which returns while its input does
    not exist yet (asserted: the event behind the copy has not completed) --, then copies of output and status, then
    the input, the output and the status overwritten.  The copies hold the oracle's result.  The default stream is the
    legacy null stream and the context's own streams are non-blocking: nothing orders them but the library's events."""
    step = S.BY_NAME[name]
    s = stream_of(kind)
    a_src = device_input(step)
    a_dev, out, kept, warm = (garbage_like(a_src) for _ in range(4))
    st, kept_st, warm_st = (garbage_status(step) for _ in range(3))
    fed = torch.cuda.Event()
    inv = g.Inverter(algo="auto")
    try:
        with torch.cuda.stream(s):
            enqueue(inv, monkeypatch, step, a_src, warm, warm_st)   # sizes the workspace: no growth hides the race
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            t0 = time.perf_counter()
            delay.enqueue()
            a_dev.copy_(a_src)
            fed.record()
            t1 = time.perf_counter()
            enqueue(inv, monkeypatch, step, a_dev, out, st)
            pending = not fed.query()
            t2 = time.perf_counter()
            kept.copy_(out)
            kept_st.copy_(st)
            a_dev.fill_(float("nan"))
            out.zero_()
            st.fill_(-1)
        torch.cuda.synchronize()
    finally:
        inv.close()
    print(f"\n[sequences] B {name} on the {kind} stream: call enqueued in {(t2 - t1) * 1e3:.2f} ms, {(t2 - t0) * 1e3:.2f} ms "
          f"after the {delay.ms:.1f} ms delay was; input still pending: {pending}")
    # (N = 4200, several hundred launches, included: measured 1.8 ms of host time against the 50 ms delay)
    assert pending, "the library returned only after its input was produced: the test proves nothing"
    check(oracle, step, kept, kept_st, f"B {kind}")
    assert torch.equal(kept_st, warm_st)
    ok = [b for b, v in enumerate(step.status) if v == S.STATUS_OK]
    assert torch.equal(kept.view(step.batch, step.n, step.n)[ok], warm.view(step.batch, step.n, step.n)[ok])   # extra
    assert bool(torch.isnan(a_dev).all()) and not bool(out.any()) and st.tolist() == [-1] * step.batch


# ---- C. changing streams under load -----------------------------------------------------------------------------------
def prepared(steps):
    """Input, output and status of every step, allocated and filled before the first call."""
    return {s.name: (device_input(s), garbage_like(device_input(s)), garbage_status(s)) for s in steps}


@pytest.mark.parametrize("long_name", [S.SPLIT.name, "tall-base"])
def test_a_small_call_on_another_stream_right_behind_a_long_one(oracle, monkeypatch, delay, long_name):
    """A long call on s1 (behind a delay, so that it is certainly still pending), then at once N = 130 on s2, which
    carves the head of the workspace the long call is using: the switch event of mi32_set_stream is all that orders
    them.  The long call is the split batch (the second half writes the caller's buffers from a private stream) in one
    variant and N = 4200 (look-ahead half on the second stream) in the other."""
    long, small = S.BY_NAME[long_name], S.BY_NAME["c-130-a"]
    t = prepared([long, small])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    done1 = torch.cuda.Event()
    inv = g.Inverter(algo="auto")
    try:
        inv.reserve(long.n, long.batch)   # no growth, whose synchronisation would order the calls
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            delay.enqueue()
            enqueue(inv, monkeypatch, long, *t[long.name])
            done1.record()
        with torch.cuda.stream(s2):
            enqueue(inv, monkeypatch, small, *t[small.name])
        pending = not done1.query()
        torch.cuda.synchronize()
    finally:
        inv.close()
    print(f"\n[sequences] C(a) {long_name}: long call still pending when the small one was enqueued: {pending}")
    assert pending
    check(oracle, long, *t[long.name][1:], "C(a) long")
    check(oracle, small, *t[small.name][1:], "C(a) small")


@pytest.mark.parametrize("long_name", [S.SPLIT.name, "tall-base"])
def test_a_long_call_on_another_stream_right_behind_a_pending_small_one(oracle, monkeypatch, delay, long_name):
    """The reverse: N = 130 behind a delay on s1, then the long call on s2 -- its first kernels, and its second
    stream's, would run over the small call's workspace at once but for the switch event."""
    long, small = S.BY_NAME[long_name], S.BY_NAME["c-130-b"]
    t = prepared([long, small])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    done1 = torch.cuda.Event()
    inv = g.Inverter(algo="auto")
    try:
        inv.reserve(long.n, long.batch)
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            delay.enqueue()
            enqueue(inv, monkeypatch, small, *t[small.name])
            done1.record()
        with torch.cuda.stream(s2):
            enqueue(inv, monkeypatch, long, *t[long.name])
        pending = not done1.query()
        torch.cuda.synchronize()
    finally:
        inv.close()
    print(f"\n[sequences] C(b) {long_name}: small call still pending when the long one was enqueued: {pending}")
    assert pending
    check(oracle, small, *t[small.name][1:], "C(b) small")
    check(oracle, long, *t[long.name][1:], "C(b) long")


def test_a_stream_of_torch_then_the_default_stream_then_the_first_again(oracle, monkeypatch, delay):
    """s1 -> the default stream -> s1, a small call each time, the first behind a delay: three calls over the same
    bytes of the workspace, ordered by two switch events (one of them on the null stream)."""
    steps = [S.BY_NAME[k] for k in ("c-130-a", "c-130-b", "c-130-c")]
    t = prepared(steps)
    s1 = torch.cuda.Stream()
    done1 = torch.cuda.Event()
    inv = g.Inverter(algo="auto")
    try:
        inv.reserve(steps[0].n, 1)
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            delay.enqueue()
            enqueue(inv, monkeypatch, steps[0], *t[steps[0].name])
            done1.record()
        with torch.cuda.stream(torch.cuda.default_stream()):
            enqueue(inv, monkeypatch, steps[1], *t[steps[1].name])
        with torch.cuda.stream(s1):
            enqueue(inv, monkeypatch, steps[2], *t[steps[2].name])
        pending = not done1.query()
        torch.cuda.synchronize()
    finally:
        inv.close()
    print(f"\n[sequences] C(c): first call still pending when the third was enqueued: {pending}")
    assert pending
    for s in steps:
        check(oracle, s, *t[s.name][1:], "C(c)")
