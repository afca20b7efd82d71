"""Host-only tests of the Python side of the relaxation calls: every ValueError of ``Inverter.csr_block_residual`` and
``Inverter.relax_stored``, raised before an address is formed -- an ``Inverter`` without a handle (its device set to the
CPU), a plain namespace for the plan and CPU tensors, in the manner of tests/test_stored_args.py -- and the host checks
they are made of.  No library call, no GPU."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gpu_matrix_inversion_amd as g
from gpu_matrix_inversion_amd.api import Inverter, StoredInverses, check_blocks_disjoint, check_sweeps

CPU = torch.device("cpu")
ORDERS = [4, 9, 70]
N = sum(ORDERS)


def plan_of(orders=ORDERS, device=CPU, p=1):
    o = np.asarray(orders, np.int32)
    return SimpleNamespace(batch=int(o.size), flat_size=int((o.astype(np.int64) ** 2).sum()), total_rows=int(o.sum()),
                           orders=o, device=device, _p=p)


def stored_of(plan, dtype=torch.float32):
    return StoredInverses(plan, dtype, torch.zeros(plan.batch, dtype=torch.int32), torch.zeros(plan.batch, dtype=torch.int64),
                          torch.zeros(8 * plan.flat_size, dtype=torch.uint8), 8 * plan.flat_size, 4 * plan.flat_size,
                          (plan.batch, 0, 0, 0))


def csr(n=N, dtype=torch.float32, index=torch.int32):
    """The identity in CSR."""
    return (torch.arange(n + 1, dtype=index), torch.arange(n, dtype=index), torch.ones(n, dtype=dtype))


def refused(match, fn, *args, **kw):
    with pytest.raises(ValueError, match=match):
        fn(*args, **kw)


@pytest.fixture
def inv():
    """An Inverter that never saw a device: every refusal must come before the first library call."""
    i = Inverter.__new__(Inverter)
    i._torch, i.device, i._h, i._diag_plan = torch, CPU, None, None
    return i


def test_methods_are_public():
    assert "Inverter" in g.__all__
    for name in ("csr_block_residual", "relax_stored"):
        assert callable(getattr(g.Inverter, name))


def test_disjoint_blocks_and_sweeps():
    check_blocks_disjoint([0, 4, 13], ORDERS)
    check_blocks_disjoint([20, 0, 100], ORDERS)            # any order, gaps allowed
    check_blocks_disjoint([13, 0, 4], [70, 4, 9])
    refused("overlap", check_blocks_disjoint, [0, 3, 13], ORDERS)
    refused("overlap", check_blocks_disjoint, [0, 4, 12], ORDERS)
    refused("blocks 1 .* and 0", check_blocks_disjoint, [5, 0, 100], [4, 9, 70])
    refused("overlap", check_blocks_disjoint, [7, 7, 100], [1, 1, 5])
    assert check_sweeps(3, 1) == (3, 1.0) and check_sweeps(np.int64(1), np.float32(0.5)) == (1, 0.5)
    for bad in (0, -1, 1.0, True, "2", None):
        refused("sweeps", check_sweeps, bad, 1.0)
    for bad in ("1", None, True, 1j):
        refused("omega", check_sweeps, 1, bad)


def _vectors(n=N, dtype=torch.float32):
    return torch.zeros(n, dtype=dtype), torch.ones(n, dtype=dtype)


def test_csr_block_residual_refusals(inv):
    plan, a = plan_of(), csr()
    x, b = _vectors()
    call = inv.csr_block_residual
    refused("open RaggedPlan", call, a, plan_of(p=None), x, b)
    refused("the plan lives on", call, a, plan_of(device=torch.device("meta")), x, b)
    refused("sparse_csr tensor or a", call, torch.eye(N), plan, x, b)
    refused("expected one index dtype", call, (a[0], a[1].long(), a[2]), plan, x, b)
    refused("block_orders sum to", call, csr(N + 1), plan, *_vectors(N + 1))
    refused("leaves the matrix", call, a, plan, x, b, first_rows=[0, 4, 14])
    refused("first_rows: a 1-D integer sequence", call, a, plan, x, b, first_rows=[0, 4])
    # x and b: a tensor of the values' dtype and device, N entries, contiguous
    refused("x: expected a tensor", call, a, plan, np.zeros(N, np.float32), b)
    refused("b: expected a tensor", call, a, plan, x, None)
    refused("x is torch.float64", call, a, plan, x.double(), b)
    refused("b is torch.float64", call, a, plan, x, b.double())
    refused("x is on meta", call, a, plan, x.to("meta"), b)
    refused("x: expected a contiguous 1-D tensor of 83 entries", call, a, plan, torch.zeros(N + 1), b)
    refused("b: expected a contiguous 1-D tensor", call, a, plan, x, torch.ones(2 * N)[::2])
    refused("x: expected a contiguous 1-D tensor", call, a, plan, torch.zeros(N, 1), b)
    # out: dtype, device, length, contiguity, overlap with everything read
    refused("out: expected a tensor", call, a, plan, x, b, out=[0.0] * N)
    refused("out is torch.float64", call, a, plan, x, b, out=torch.zeros(N, dtype=torch.float64))
    refused("out is on meta", call, a, plan, x, b, out=torch.zeros(N, device="meta"))
    refused("out: expected a contiguous 1-D tensor of 83 entries", call, a, plan, x, b, out=torch.zeros(N - 1))
    refused("out: expected a contiguous 1-D tensor", call, a, plan, x, b, out=torch.zeros(2 * N)[::2])
    refused("out must not alias x", call, a, plan, x, b, out=x)
    refused("out must not alias b", call, a, plan, x, b, out=b)
    refused("out must not alias values", call, a, plan, x, b, out=a[2])
    both = torch.zeros(2 * N - 1)
    refused("out must not alias x", call, a, plan, both[:N], b, out=both[N - 1:])


def test_relax_stored_refusals(inv):
    plan, a = plan_of(), csr()
    stored = stored_of(plan)
    x, b = _vectors()
    call = inv.relax_stored
    refused("expected the StoredInverses", call, a, plan, x, b)
    refused("stored holds torch.float32 members, the matrix is torch.float64", call, csr(dtype=torch.float64), stored,
            *_vectors(dtype=torch.float64))
    refused("stored holds torch.float64", call, a, stored_of(plan, torch.float64), x, b)
    refused("open RaggedPlan", call, a, stored_of(plan_of(p=None)), x, b)
    refused("sweeps", call, a, stored, x, b, sweeps=0)
    refused("sweeps", call, a, stored, x, b, sweeps=1.5)
    refused("omega", call, a, stored, x, b, omega="1")
    refused("block_orders sum to", call, csr(N + 1), stored, *_vectors(N + 1))
    # blocks must not overlap one another, decided on the host
    refused("overlap", call, csr(200), stored, *_vectors(200), first_rows=[0, 3, 13])
    refused("overlap", call, csr(200), stored, *_vectors(200), first_rows=[100, 60, 50])
    refused("leaves the matrix", call, csr(200), stored, *_vectors(200), first_rows=[0, 4, 131])
    refused("x is torch.float64", call, a, stored, x.double(), b)
    refused("b: expected a contiguous 1-D tensor of 83 entries", call, a, stored, x, torch.ones(N + 2))
    refused("x: expected a contiguous 1-D tensor", call, a, stored, torch.zeros(2 * N)[::2], b)
    refused("out is torch.float64", call, a, stored, x, b, out=torch.zeros(N, dtype=torch.float64))
    refused("out: expected a contiguous 1-D tensor of 83 entries", call, a, stored, x, b, out=torch.zeros(N + 1))
    refused("out: expected a contiguous 1-D tensor", call, a, stored, x, b, out=torch.zeros(2 * N)[::2])
    refused("out is on meta", call, a, stored, x, b, out=torch.zeros(N, device="meta"))
    refused("out must not alias x", call, a, stored, x, b, out=x)
    refused("out must not alias b", call, a, stored, x, b, out=b)
    refused("out must not alias values", call, a, stored, x, b, out=a[2])
    # the index arrays and the store are bytes of another dtype: views of one buffer stand for the overlap
    raw = torch.zeros(4 * N + 8 * plan.flat_size, dtype=torch.uint8)
    over = StoredInverses(plan, torch.float32, stored.formats, stored.offsets, raw, stored.nbytes, stored.native_nbytes,
                          stored.counts)
    refused(r"out must not alias stored\.data", call, a, over, x, b, out=raw[:4 * N].view(torch.float32))
    words = torch.zeros(2 * N + 1, dtype=torch.int32)
    refused("out must not alias crow", call, (words[:N + 1], a[1], a[2]), stored, x, b, out=words[N:].view(torch.float32)[:N])
    refused("out must not alias col", call, (a[0], words[:N], a[2]), stored, x, b, out=words[1:N + 1].view(torch.float32))
