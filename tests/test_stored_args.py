"""Host-only tests of the Python side of the stored inverses: ``api.choose_storage`` on CPU tensors against the NumPy
restatement (tests/stored_cases.py) with every branch of the rule taken, ``STORAGE_FORMATS``, ``stored_layout``, and
every ValueError of ``block_stats*`` / ``store_inverses*`` / ``apply_stored``, raised before an address is formed: an
``Inverter`` without a handle (its device set to the CPU) and a plain namespace for the plan, in the manner of
tests/test_ragged_args.py.  No library call, no GPU."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import stored_cases as sc
import gpu_matrix_inversion_amd as g
from gpu_matrix_inversion_amd.api import (STORAGE_FORMATS, Inverter, StoredInverses, check_storage_formats, choose_storage,
                                          stored_layout)

CPU = torch.device("cpu")
ORDERS = [4, 9, 70]


def plan_of(orders=ORDERS, device=CPU, p=1):
    o = np.asarray(orders, np.int32)
    return SimpleNamespace(batch=int(o.size), flat_size=int((o.astype(np.int64) ** 2).sum()), total_rows=int(o.sum()),
                           orders=o, device=device, _p=p)


PLAN = plan_of()


def refused(match, fn, *args, **kw):
    with pytest.raises(ValueError, match=match):
        fn(*args, **kw)


@pytest.fixture
def inv():
    """An Inverter that never saw a device: every refusal must come before the first library call."""
    i = Inverter.__new__(Inverter)
    i._torch, i.device, i._h, i._diag_plan = torch, CPU, None, None
    return i


def test_public_names_and_format_table():
    for name in ("STORAGE_FORMATS", "StoredInverses", "choose_storage"):
        assert name in g.__all__ and hasattr(g, name)
    assert sorted(STORAGE_FORMATS) == [0, 1, 2, 3]
    assert [STORAGE_FORMATS[c].name for c in range(4)] == ["native", "float32", "float16", "bfloat16"]
    assert [STORAGE_FORMATS[c].nbytes for c in range(4)] == [None, 4, 2, 2]
    for code, (u, small, large) in sc.LIMITS.items():
        f = STORAGE_FORMATS[code]
        assert (f.u, f.smallest_normal, f.largest_finite) == (u, small, large)
    assert STORAGE_FORMATS[2].largest_finite == float(np.finfo(np.float16).max)
    assert STORAGE_FORMATS[2].smallest_normal == float(np.finfo(np.float16).tiny)
    assert STORAGE_FORMATS[1].largest_finite == float(np.finfo(np.float32).max)
    assert STORAGE_FORMATS[3].largest_finite == float(torch.finfo(torch.bfloat16).max)
    assert STORAGE_FORMATS[3].u == torch.finfo(torch.bfloat16).eps / 2


# (kappa, absmax, absmin, status): the branch it takes, for float32 and float64 members
BRANCHES = [
    (10.0, 100.0, 1e-3, 0, 2, 2),               # float16
    (0.1 / 2.0 ** -11, 65504.0, 2.0 ** -14, 0, 2, 2),   # float16 at all three edges
    (0.1 / 2.0 ** -11 * (1 + 2.0 ** -40), 1.0, 1.0, 0, 0, 1),  # kappa a hair too large for float16 AND bfloat16
    (10.0, 65505.0, 1e-3, 0, 3, 3),             # absmax past float16: bfloat16
    (10.0, 100.0, 2.0 ** -15, 0, 3, 3),         # absmin below float16's normals: bfloat16
    (0.1 / 2.0 ** -8, 1e30, 1e-30, 0, 3, 3),    # bfloat16 at its kappa edge
    (26.0, 1e30, 1e-30, 0, 0, 1),               # kappa past bfloat16: float32 for fp64, native for fp32
    (1e3, 1.0, 1.0, 0, 0, 1),
    (0.1 / 2.0 ** -24, 1.0, 1.0, 0, 0, 1),      # float32 at its kappa edge
    (1e8, 1.0, 1.0, 0, 0, 0),                   # past float32: native
    (10.0, 1e39, 1.0, 0, 0, 0),                 # absmax past bfloat16 and float32
    (10.0, 1.0, 1e-40, 0, 0, 0),                # absmin subnormal in float32 and bfloat16
    (np.inf, 1.0, 1.0, 0, 0, 0),                # a non-finite kappa
    (np.nan, np.nan, np.nan, 0, 0, 0),
    (10.0, 100.0, 1e-3, 2, 0, 0),               # a singular member
    (10.0, 100.0, 1e-3, -1, 0, 0),
    (0.0, 0.0, np.inf, 0, 2, 2),                # an all-zero inverse
    (10.0, np.inf, 1.0, 0, 0, 0),               # an infinity inside
]


def test_choose_storage_takes_every_branch():
    k, big, small, st = (np.array([b[i] for b in BRANCHES], np.float64) for i in range(4))
    st = st.astype(np.int32)
    for dtype, col in ((torch.float32, 4), (torch.float64, 5)):
        want = np.array([b[col] for b in BRANCHES], np.int32)
        np_dtype = np.float32 if dtype == torch.float32 else np.float64
        assert np.array_equal(sc.choose(np_dtype, k, big, small, 0.1, st), want)       # the restatement, by hand
        got = choose_storage(dtype, torch.from_numpy(k), torch.from_numpy(big), torch.from_numpy(small), 0.1,
                             torch.from_numpy(st))
        assert got.dtype == torch.int32 and got.device == CPU and np.array_equal(got.numpy(), want)
        assert set(want.tolist()) == ({0, 2, 3} if col == 4 else {0, 1, 2, 3})
    # without a status the singular members are judged by their numbers; tol moves the edges
    got = choose_storage(torch.float64, torch.from_numpy(k), torch.from_numpy(big), torch.from_numpy(small))
    assert np.array_equal(got.numpy(), sc.choose(np.float64, k, big, small)) and got[14] == 2
    for tol in (1e-3, 1.0, 2.0 ** -11 * 10):
        got = choose_storage(torch.float64, torch.from_numpy(k), torch.from_numpy(big), torch.from_numpy(small), tol,
                             torch.from_numpy(st))
        assert np.array_equal(got.numpy(), sc.choose(np.float64, k, big, small, tol, st)), tol


def test_choose_storage_on_random_statistics():
    rng = np.random.default_rng(3)
    n = 4000
    k = 10.0 ** rng.uniform(-1, 10, n)
    big = 10.0 ** rng.uniform(-3, 42, n)
    small = big * 10.0 ** -rng.uniform(0, 12, n)
    st = (rng.uniform(size=n) < 0.05).astype(np.int32) * 3
    k[::97] = np.inf
    for dtype, np_dtype in ((torch.float32, np.float32), (torch.float64, np.float64)):
        got = choose_storage(dtype, torch.from_numpy(k), torch.from_numpy(big), torch.from_numpy(small), 0.1,
                             torch.from_numpy(st))
        assert np.array_equal(got.numpy(), sc.choose(np_dtype, k, big, small, 0.1, st))


def test_choose_storage_refusals():
    v = torch.ones(3, dtype=torch.float64)
    choose_storage(torch.float32, v, v, v)
    refused("dtype: expected torch.float32 or torch.float64", choose_storage, torch.float16, v, v, v)
    refused("kappa: expected a 1-D float64 tensor", choose_storage, torch.float32, v.float(), v, v)
    refused("absmax: expected a 1-D float64 tensor", choose_storage, torch.float32, v, v.numpy(), v)
    refused("absmin: expected a 1-D float64 tensor", choose_storage, torch.float32, v, v, v.reshape(3, 1))
    refused("absmax: expected kappa's length and device", choose_storage, torch.float32, v, v[:2], v)
    refused("absmin: expected kappa's length and device", choose_storage, torch.float32, v, v, v.to("meta"))
    for tol in (0, -1.0, float("inf"), float("nan"), None, "0.1"):
        refused("tol: a positive finite number", choose_storage, torch.float32, v, v, v, tol)
    refused("status: an integer tensor", choose_storage, torch.float32, v, v, v, 0.1, v)
    refused("status: an integer tensor", choose_storage, torch.float32, v, v, v, 0.1, torch.zeros(2, dtype=torch.int32))
    refused("status: an integer tensor", choose_storage, torch.float32, v, v, v, 0.1, [0, 0, 0])


def test_format_codes_are_checked_on_the_host():
    assert check_storage_formats(PLAN, torch.float32, [0, 2, 3]).tolist() == [0, 2, 3]
    got = check_storage_formats(PLAN, torch.float64, torch.tensor([1, 2, 3], dtype=torch.int32))
    assert got.dtype == np.int32 and got.tolist() == [1, 2, 3]
    assert check_storage_formats(PLAN, torch.float64, np.array([0, 1, 0], np.int64)).tolist() == [0, 1, 0]
    refused("formats: a 1-D integer sequence of 3 entries", check_storage_formats, PLAN, torch.float32, [0, 2])
    refused("formats: a 1-D integer sequence of 3 entries", check_storage_formats, PLAN, torch.float32, [[0, 2, 3]])
    refused("formats: a 1-D integer sequence of 3 entries", check_storage_formats, PLAN, torch.float32, [0.0, 2.0, 3.0])
    refused("formats is torch.int64, expected torch.int32", check_storage_formats, PLAN, torch.float32,
            torch.tensor([0, 2, 3]))
    refused("member 1 has code 1, which torch.float32 members do not take", check_storage_formats, PLAN, torch.float32,
            [0, 1, 3])
    refused("member 2 has code 4", check_storage_formats, PLAN, torch.float64, [0, 1, 4])
    refused("member 0 has code -1", check_storage_formats, PLAN, torch.float64, [-1, 1, 2])
    refused("dtype: expected torch.float32 or torch.float64", check_storage_formats, PLAN, torch.float16, [0, 2, 3])


def test_layout_is_the_restatement():
    rng = np.random.default_rng(5)
    orders = rng.integers(1, 129, 300)
    for dtype in (np.float32, np.float64):
        formats = rng.choice(sc.codes_of(dtype), orders.size)
        off, size = stored_layout(orders, formats, np.dtype(dtype).itemsize)
        want_off, want_size = sc.offsets(orders, formats, dtype)
        assert off.dtype == np.int64 and np.array_equal(off, want_off) and size == want_size
        assert (off % 8 == 0).all() and size % 8 == 0
    off, size = stored_layout([3, 1, 2, 5], [2, 0, 3, 1], 8)
    assert off.tolist() == [0, 24, 32, 40] and size == 144
    # 32 768 members of order 64 in float64: the offsets leave 32 bits
    off, size = stored_layout(np.full(32_768, 64), np.zeros(32_768, np.int64), 8)
    assert size == 2 ** 30 and off[-1] == 2 ** 30 - 64 * 64 * 8


def test_block_stats_refusals(inv):
    flat = torch.zeros(PLAN.flat_size)
    refused("expected an open RaggedPlan", inv.block_stats, plan_of(p=None), flat)
    refused("the plan lives on meta", inv.block_stats, plan_of(device=torch.device("meta")), flat)
    refused("dtype: expected torch.float32 or torch.float64", inv.block_stats, PLAN, flat.half())
    refused("flat: expected a contiguous 1-D tensor of 4997 entries", inv.block_stats, PLAN, flat[:-1])
    refused("flat is on meta", inv.block_stats, PLAN, flat.to("meta"))
    refused("flat: expected a contiguous 1-D tensor", inv.block_stats, PLAN, torch.zeros(2 * PLAN.flat_size)[::2])
    ptrs = torch.zeros(3, dtype=torch.int64)
    refused("expected an open RaggedPlan", inv.block_stats_pointers, None, ptrs, torch.float32)
    refused("dtype: expected torch.float32 or torch.float64", inv.block_stats_pointers, PLAN, ptrs, torch.int32)
    refused("ptrs is torch.int32, expected torch.int64", inv.block_stats_pointers, PLAN, ptrs.int(), torch.float32)
    refused("ptrs: expected a contiguous 1-D tensor of 3 entries", inv.block_stats_pointers, PLAN, ptrs[:2], torch.float32)
    refused("ld is torch.int64, expected torch.int32", inv.block_stats_pointers, PLAN, ptrs, torch.float32, ptrs)
    refused("ld: expected a contiguous 1-D tensor of 3 entries", inv.block_stats_pointers, PLAN, ptrs, torch.float32,
            torch.zeros(4, dtype=torch.int32))
    refused("orders up to 128", inv.block_stats_pointers, plan_of([4, 129]), ptrs[:2], torch.float32)


def test_store_inverses_refusals(inv):
    x = torch.zeros(PLAN.flat_size)
    refused("expected an open RaggedPlan", inv.store_inverses, plan_of(p=None), x, [0, 0, 0])
    refused("dtype: expected torch.float32 or torch.float64", inv.store_inverses, PLAN, x.half(), [0, 0, 0])
    refused("x_flat: expected a contiguous 1-D tensor of 4997 entries", inv.store_inverses, PLAN, x[1:], [0, 0, 0])
    refused("formats: a 1-D integer sequence of 3 entries", inv.store_inverses, PLAN, x, [0, 0])
    refused("member 0 has code 1, which torch.float32 members do not take", inv.store_inverses, PLAN, x, [1, 0, 0])
    refused("member 2 has code 7", inv.store_inverses, PLAN, x.double(), [1, 0, 7])
    refused("formats is torch.float32, expected torch.int32", inv.store_inverses, PLAN, x, torch.zeros(3))
    size = stored_layout(ORDERS, [2, 0, 3], 4)[1]
    refused("data is torch.float32, expected torch.uint8", inv.store_inverses, PLAN, x, [2, 0, 3], data=torch.zeros(size))
    refused("data: at least %d bytes" % size, inv.store_inverses, PLAN, x, [2, 0, 3],
            data=torch.zeros(size - 8, dtype=torch.uint8))
    refused("data: at least %d bytes at an address that is a multiple of 8" % size, inv.store_inverses, PLAN, x, [2, 0, 3],
            data=torch.zeros(size + 8, dtype=torch.uint8)[1:])
    refused("data is on meta", inv.store_inverses, PLAN, x, [2, 0, 3], data=torch.zeros(size, dtype=torch.uint8, device="meta"))
    refused("data must not alias x_flat", inv.store_inverses, PLAN, x, [2, 0, 3], data=x.view(torch.uint8))
    ptrs = torch.zeros(3, dtype=torch.int64)
    refused("x_ptrs is torch.int32", inv.store_inverses_pointers, PLAN, ptrs.int(), torch.float32, [0, 0, 0])
    refused("ldx is torch.int64", inv.store_inverses_pointers, PLAN, ptrs, torch.float32, [0, 0, 0], ptrs)
    refused("member 1 has code 1", inv.store_inverses_pointers, PLAN, ptrs, torch.float32, [0, 1, 0])
    refused("dtype: expected torch.float32 or torch.float64", inv.store_inverses_pointers, PLAN, ptrs, torch.bfloat16, [0, 0, 0])


def stored_of(plan=PLAN, dtype=torch.float32, nbytes=4096):
    z = torch.zeros(plan.batch, dtype=torch.int32)
    return StoredInverses(plan, dtype, z, z.long(), torch.zeros(nbytes, dtype=torch.uint8), nbytes, plan.flat_size * 4,
                          (plan.batch, 0, 0, 0))


def test_apply_stored_refusals(inv):
    st = stored_of()
    r = torch.zeros(PLAN.total_rows, 2)
    refused("expected the StoredInverses of store_inverses", inv.apply_stored, torch.zeros(PLAN.flat_size), r)
    refused("expected the StoredInverses of store_inverses", inv.apply_stored, None, r)
    refused("expected an open RaggedPlan", inv.apply_stored, stored_of(plan_of(p=None)), r)
    refused("the plan lives on meta", inv.apply_stored, stored_of(plan_of(device=torch.device("meta"))), r)
    refused("r is torch.float64 on cpu, expected torch.float32 on cpu", inv.apply_stored, st, r.double())
    refused("r is torch.float32 on cpu, expected torch.float64 on cpu", inv.apply_stored, stored_of(dtype=torch.float64), r)
    refused("r is torch.float32 on meta", inv.apply_stored, st, r.to("meta"))
    refused(r"r: expected \(83,\) or \(83, K\)", inv.apply_stored, st, r[:-1])
    refused(r"r: expected \(83,\) or \(83, K\)", inv.apply_stored, st, torch.zeros(PLAN.total_rows, 0))
    refused(r"r: expected \(83,\) or \(83, K\)", inv.apply_stored, st, torch.zeros(PLAN.total_rows, 2, 2))
    refused("out: r itself or a contiguous tensor of its shape", inv.apply_stored, st, r, torch.zeros(PLAN.total_rows, 3))
    refused("out: r itself or a contiguous tensor of its shape", inv.apply_stored, st, r, r.double())
    base = torch.zeros(PLAN.total_rows * 2 + 2)
    refused("out may be the input it replaces", inv.apply_stored, st, base[:-2].view(-1, 2), base[2:].view(-1, 2))
    # out inside the store's bytes, as a view of them
    inside = st.data[:PLAN.total_rows * 2 * 4].view(torch.float32).reshape(PLAN.total_rows, 2)
    refused("out must not alias the matrices", inv.apply_stored, st, r, inside)
    refused("out must not alias the matrices", inv.apply_stored, st, inside, inside)
