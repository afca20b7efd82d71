"""Back-to-back calls on ONE context (tests/test_sequence_cases.py pins the plans and the oracle's statuses without a
device, tests/test_gpu_sequences.py runs the sequences on the GPU).  Pure numpy, seeded; no device anywhere in this file.

A step is one call: its route, dtype, order, batch and the settings it needs on the live handle.  Every route has one
oracle function and one comparison, the ones the single-call tests of that route already use:

  route        oracle                                                  comparison
  blocked32    matrix_inv_32_inplace (<= 1024) / _blocked_exact        conftest.canonical_bytes
  nopivot32    matrix_inversion_no_pivots (float32)                    conftest.canonical_bytes
  sweep32      matrix_inv_32                                           np.array_equal
  sweep64      matrix_inv_64                                           np.array_equal
  blocked64    matrix_inv_64_blocked at the resolved block width       np.array_equal
  nopivot64    matrix_inversion_no_pivots (float64)                    np.array_equal
  residual     residual_inf / residual_inf_left / frobenius_metric     rel 1e-9 / 1e-9 / 1e-6 (the only tolerance)

A flagged member has no expected values (None): only its status word is compared.
"""
import collections

import numpy as np

import nopivot_cases
import tall_batch_cases as T
from conftest import canonical_bytes, gate_matrix

ALGO_AUTO, ALGO_SWEEP, ALGO_BLOCKED = 0, 1, 2
STATUS_OK, STATUS_SINGULAR = 0, 2
BYTES_ROUTES = ("blocked32", "nopivot32")   # zero multipliers are multiplied through: the sign of a zero may differ

# name; route; numpy dtype; order; batch; pivoting and algorithm to set on the live handle; the algorithm the library
# must resolve the call to; the statuses expected; environment of this call only
Step = collections.namedtuple("Step", "name route dtype n batch pivoting algo resolves status env")


def _step(name, route, n, batch=1, pivoting=True, algo=ALGO_AUTO, status=None, env=None):
    dtype = np.float64 if route.endswith("64") else np.float32
    resolves = ALGO_SWEEP if route.startswith("sweep") else ALGO_BLOCKED
    return Step(name, route, dtype, n, batch, pivoting, algo, resolves, status or [STATUS_OK] * batch, env or {})


LOOKAHEAD_ENV = {"MI32_LOOKAHEAD_MIN": "2048"}   # read per call in plan_route

# ---- S1: every route of a context, each step behind one of another kind ------------------------------------------------
S1 = [
    _step("1", "blocked64", 300),                                 # the fp64 cross-over is 256
    _step("2", "blocked32", 200, status=[STATUS_SINGULAR]),       # one NaN entry: non-finite values stay in the workspace
    _step("3a", "blocked32", 130),                                # 256 padded rows: one outer block
    _step("3b", "blocked32", 300),                                # two blocks
    _step("4a", "sweep32", 20),                                   # AUTO below 32
    _step("4b", "sweep32", 300, algo=ALGO_SWEEP),
    _step("5", "sweep64", 100),
    _step("6", "blocked32", 160, batch=3, status=[STATUS_OK, STATUS_SINGULAR, STATUS_OK]),
    _step("7a", "nopivot32", 600, pivoting=False),                # the no-pivot cross-over is 512
    _step("7b", "nopivot64", 600, pivoting=False),
    _step("8r", "residual", 300),                                 # on step 3b's pair; memsets the head of the workspace
    _step("8", "blocked32", 300),                                 # another matrix than 3b's
    _step("9", "blocked32", 300),                                 # step 3b's call again
]
SAME_INPUT = {"9": "3b", "8r": "3b"}

# ---- S2: the tall sequence --------------------------------------------------------------------------------------------
N_TALL = T.N_TALL
S2 = [
    _step("tall-base", "blocked32", N_TALL),                      # shared two-workgroup panels and the look-ahead
    _step("la-2048", "blocked32", 2048, env=LOOKAHEAD_ENV),       # 2048 padded rows: the smallest look-ahead shape
    _step("small-130", "blocked32", 130),
    _step("tall-variant", "blocked32", N_TALL),
    _step("tall-pair", "blocked32", N_TALL, batch=2),             # shared panels with a batch index, tags from 1 again
]

# ---- the split batch of sections B and C --------------------------------------------------------------------------------
SPLIT_N, SPLIT_BATCH = 1024, 65            # 33 + 32 members, 65 Mi elements, block width 128
SPLIT_ORACLE_MEMBERS = (0, 32, 33, 64)     # the first and last member of either half: compared with the oracle itself
SPLIT_SINGULAR = (5, 60)                   # one in either half
SPLIT = _step("split-65x1024", "blocked32", SPLIT_N, batch=SPLIT_BATCH,
              status=[STATUS_SINGULAR if b in SPLIT_SINGULAR else STATUS_OK for b in range(SPLIT_BATCH)])

# the single calls of sections B and C that S1 and S2 do not hold already
EXTRA = {s.name: s for s in (SPLIT, _step("c-130-a", "blocked32", 130), _step("c-130-b", "blocked32", 130),
                             _step("c-130-c", "blocked32", 130))}
BY_NAME = {s.name: s for s in S1 + S2 + list(EXTRA.values())}

# what mi32_resolve_route must say of a step for the step to be the test it is meant to be (fields of mi32_route_t)
ROUTE_FACTS = {
    "2": {"nblocks": 1}, "3a": {"np": 256, "nblocks": 1}, "3b": {"np": 384, "nblocks": 2}, "6": {"parts": 1},
    "8": {"nblocks": 2}, "9": {"nblocks": 2}, "7a": {"np": 640, "lookahead": 0},
    "tall-base": {"np": 4224, "shared_panels": 1, "lookahead": 1, "parts": 1},
    "tall-variant": {"np": 4224, "shared_panels": 1, "lookahead": 1, "parts": 1},
    "tall-pair": {"shared_panels": 1, "lookahead": 0, "parts": 1},
    "la-2048": {"np": 2048, "shared_panels": 0, "lookahead": 1},
    "small-130": {"nblocks": 1, "lookahead": 0}, "c-130-a": {"nblocks": 1}, "c-130-b": {"nblocks": 1}, "c-130-c": {"nblocks": 1},
    SPLIT.name: {"parts": 2, "part_batch": [33, 32], "block_width": 128, "shared_panels": 0, "lookahead": 0},
}

_SEEDS = {"1": 61_001, "2": 61_002, "3a": 61_003, "3b": 61_004, "4a": 61_005, "4b": 61_006, "5": 61_007, "6": 61_008,
          "8": 61_009, "la-2048": 61_010, "small-130": 61_011, "c-130-a": 61_012, "c-130-b": 61_013, "c-130-c": 61_014}

_INPUTS = {}
_EXPECTED = {}


def _tall_members():
    """(base, variant): the gate base of tests/tall_batch_cases.py and its 2^40-scaled, row-permuted, sign-flipped
    variant, whose inverse follows from the base's bit for bit: one oracle run serves every tall step."""
    ms = T.tall_batch(N_TALL, 3)
    assert ms[0].transform is None and ms[2].base == ms[0].base and ms[2].transform is not None
    return ms[0], ms[2]


def _split_members():
    """Members 0, 32, 33 and 64 are gate matrices of their own; member b of the others is an exact variant (2^k P a D,
    tall_batch_cases.variant) of the base b % 4, so that its status and its inverse follow from that base's; members 5
    and 60 are singular: all ones, and a zero column at step 700."""
    n = SPLIT_N
    bases = [gate_matrix(n, 62_000 + i) for i in range(4)]
    members = []
    for b in range(SPLIT_BATCH):
        if b in SPLIT_ORACLE_MEMBERS:
            members.append(T.Member(bases[SPLIT_ORACLE_MEMBERS.index(b)], SPLIT_ORACLE_MEMBERS.index(b), None))
        elif b == SPLIT_SINGULAR[0]:
            members.append(T.Member(np.ones((n, n), np.float32), None, None))
        elif b == SPLIT_SINGULAR[1]:
            a = bases[0].copy()
            a[:, 700] = 0
            members.append(T.Member(a, None, None))
        else:
            a1, t = T.variant(bases[b % 4], 63_000 + b, (3, -9, 40, -30)[b % 4])
            members.append(T.Member(a1, b % 4, t))
    return members


def split_members():
    if "split-members" not in _INPUTS:
        _INPUTS["split-members"] = _split_members()
    return _INPUTS["split-members"]


def _make_inputs(step):
    name = SAME_INPUT.get(step.name, step.name)
    n = step.n
    if name == "tall-base":
        return _tall_members()[0].matrix
    if name == "tall-variant":
        return _tall_members()[1].matrix
    if name == "tall-pair":
        return np.stack([m.matrix for m in _tall_members()])
    if name == SPLIT.name:
        return np.stack([m.matrix for m in split_members()])
    if step.route.startswith("nopivot"):                 # an SPD family: not diagonally dominant at this order
        return np.array(nopivot_cases.family("spd", n, step.dtype))
    seed = _SEEDS[name]
    if name == "2":
        a = gate_matrix(n, seed)
        a[77, 123] = np.nan
        return a
    if name == "3b":
        # The pair the residual step checks is the pair of test_device_residual_matches_oracle (U(0, 100), seed 5),
        # whose tolerance it copies: the third figure, sqrt(N) - ||AX||_F, is a difference of two numbers near 17.3,
        # and its absolute floor of 1e-12 (6e-14 of what is summed) was set on this pair.  On a gate matrix the figure
        # is -4.6e-7 and two correct double summations of different order already differ by 1.4e-12.
        return np.random.default_rng(5).uniform(0, 100, (n, n)).astype(np.float32)
    if name == "6":
        a = np.stack([gate_matrix(n, seed + b) for b in range(step.batch)])
        a[1] = 1.0
        return a
    return gate_matrix(n, seed).astype(step.dtype)


def inputs(step):
    """The input of a step, (n, n) or (batch, n, n): made once per process, read-only."""
    key = SAME_INPUT.get(step.name, step.name)
    if key not in _INPUTS:
        a = np.ascontiguousarray(_make_inputs(step))
        assert a.dtype == step.dtype and a.shape[-2:] == (step.n, step.n) and a.size == step.batch * step.n * step.n
        a.setflags(write=False)
        _INPUTS[key] = a
    return _INPUTS[key]


def members(step):
    a = inputs(step)
    return a.reshape(step.batch, step.n, step.n)


def block_width_f64(n):
    """The block width a fresh context gives the fp64 blocked path at this order (host planning, no device)."""
    import ctypes

    from gpu_matrix_inversion_amd import _lib

    bw = ctypes.c_int()
    assert _lib.load().mi32_resolve_blocking_f64(None, int(n), ctypes.byref(bw)) == _lib.MI32_OK
    return bw.value


def _oracle_member(oracle, step, a):
    n = step.n
    if step.route == "blocked32":
        fn = oracle.matrix_inv_32_inplace if n <= 1024 else (lambda m, k, **kw: oracle.matrix_inv_32_blocked_exact(m, k, 128, **kw))
    elif step.route == "sweep32":
        fn = oracle.matrix_inv_32
    elif step.route == "sweep64":
        fn = oracle.matrix_inv_64
    elif step.route == "blocked64":
        bw = block_width_f64(n)
        assert bw > 0
        fn = lambda m, k, **kw: oracle.matrix_inv_64_blocked(m, k, bw, **kw)   # noqa: E731
    elif step.route in ("nopivot32", "nopivot64"):
        fn = oracle.matrix_inversion_no_pivots
    else:
        raise ValueError(step.route)
    x, info = fn(a, n, return_info=True)
    assert x.dtype == step.dtype
    return x.reshape(n, n), int(info["status"])


def _expected(oracle, step):
    if step.name in ("tall-base", "tall-variant", "tall-pair"):
        base, var = _tall_members()
        ms = {"tall-base": [base], "tall-variant": [var], "tall-pair": [base, var]}[step.name]
        return [T.expected_inverse(oracle, m) for m in ms], [STATUS_OK] * len(ms)
    if step.name == SPLIT.name:
        ms = split_members()
        own = {}
        for b in SPLIT_ORACLE_MEMBERS + SPLIT_SINGULAR:
            own[b] = _oracle_member(oracle, step, ms[b].matrix)
        xs, sts = [], []
        for b, m in enumerate(ms):
            if b in own:
                x, st = own[b]
            else:   # an exact variant: its base's status, and the transform of its base's inverse
                x, st = own[SPLIT_ORACLE_MEMBERS[m.base]]
                x = T.apply_variant(x, m.transform)
            xs.append(x if st == STATUS_OK else None)
            sts.append(st)
        return xs, sts
    xs, sts = [], []
    for a in members(step):
        x, st = _oracle_member(oracle, step, a)
        xs.append(x if st == STATUS_OK else None)
        sts.append(st)
    return xs, sts


def expected(oracle, step):
    """(inverse of every member, None for a flagged one; status of every member) from the CPU oracle of the step's
    route: computed once per process and left unchanged."""
    assert step.route != "residual"
    key = SAME_INPUT.get(step.name, step.name)
    if key not in _EXPECTED:
        xs, sts = _expected(oracle, step)
        for x in xs:
            if x is not None:
                x.setflags(write=False)
        _EXPECTED[key] = (xs, sts)
    return _EXPECTED[key]


def expected_residual(oracle, a, x):
    """[||AX - I||_inf, ||XA - I||_inf, sqrt(N) - ||AX||_F] of the oracle on the oracle's own pair."""
    n = a.shape[0]
    return [oracle.residual_inf(a, x, n), oracle.residual_inf_left(a, x, n), oracle.frobenius_metric(a, x, n)]


def same(step, got, want):
    """The comparison of the step's route between a (n, n) result and the oracle's: bytes, no tolerance."""
    got = np.asarray(got)
    if got.dtype != step.dtype or got.shape != want.shape:
        return False
    if step.route in BYTES_ROUTES:
        return canonical_bytes(got) == canonical_bytes(want)
    return bool(np.array_equal(got, want))
