"""Host-only tests of the argument handling behind the variable-size calls (``Inverter.inv_pointers`` / ``inv_ragged`` /
``inv_diag_blocks`` and their ``solve_*`` / ``apply_*`` twins): ``api.check_ragged_call``, ``check_pointer_args``,
``check_packed_matrices``, ``check_packed_rhs``, ``check_inverse_out`` and ``check_diag_blocks``.  One assertion per
refusal and the accepted form beside it, on CPU tensors with ``device=torch.device("cpu")`` standing for the Inverter's
device, ``device="meta"`` tensors for "on another device" and a plain namespace for the plan of orders [4, 9, 70].  No
handle, no library, no GPU.  tests/test_gpu_vbatch.py, test_gpu_vsolve.py and test_gpu_apply.py repeat the refusals
through a live ``Inverter``."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gpu_matrix_inversion_amd.api import (check_diag_blocks, check_inverse_out, check_packed_matrices, check_packed_rhs,
                                          check_pointer_args, check_ragged_call)

CPU = torch.device("cpu")
ORDERS = [4, 9, 70]
BATCH, FLAT, ROWS, K = 3, 4997, 83, 2


def plan_of(orders=ORDERS, device=CPU, p=1):
    o = np.asarray(orders, np.int32)
    return SimpleNamespace(batch=int(o.size), flat_size=int((o.astype(np.int64) ** 2).sum()), total_rows=int(o.sum()),
                           orders=o, device=device, _p=p)


PLAN = plan_of()
assert (PLAN.batch, PLAN.flat_size, PLAN.total_rows) == (BATCH, FLAT, ROWS)


def refused(match, fn, *args, **kw):
    with pytest.raises(ValueError, match=match):
        fn(*args, **kw)


def ptrs(n=BATCH, dtype=torch.int64, **kw):
    return torch.zeros(n, dtype=dtype, **kw)


def pointer_args(plan=PLAN, dtype=torch.float32, p=None, lds=None, status=None, **kw):
    return check_pointer_args(CPU, plan, dtype, {"a_ptrs": ptrs()} if p is None else p, lds or {}, status, **kw)


# ---- the plan ---------------------------------------------------------------------------------------------------------
def test_plan_refusals():
    check_ragged_call(CPU, PLAN, torch.float32)
    refused("expected an open RaggedPlan", check_ragged_call, CPU, plan_of(p=None), torch.float32)         # closed
    refused("expected an open RaggedPlan", check_ragged_call, CPU, None, torch.float32)
    refused("expected an open RaggedPlan", check_ragged_call, CPU, ORDERS, torch.float32)
    refused("the plan lives on meta", check_ragged_call, CPU, plan_of(device=torch.device("meta")), torch.float32)
    # every entry point goes through it
    refused("expected an open RaggedPlan", pointer_args, plan_of(p=None))
    refused("the plan lives on meta", pointer_args, plan_of(device=torch.device("meta")))
    refused("expected an open RaggedPlan", check_packed_matrices, CPU, plan_of(p=None), torch.zeros(FLAT), "a_flat")
    refused("the plan lives on meta", check_packed_matrices, CPU, plan_of(device=torch.device("meta")), torch.zeros(FLAT),
            "a_flat")


def test_largest_order():
    with_128 = plan_of([4, 128])
    check_ragged_call(CPU, with_128, torch.float32)                                              # inv and apply take it
    check_ragged_call(CPU, plan_of([4, 127]), torch.float32, max_order=127)
    refused("orders up to 127: the plan holds an order-128 member", check_ragged_call, CPU, with_128, torch.float32,
            max_order=127)
    refused("orders up to 127", pointer_args, with_128, p={"a_ptrs": ptrs(2)}, nrhs=1, max_order=127)
    refused("orders up to 127", check_packed_matrices, CPU, with_128, torch.zeros(16 + 128 * 128), "a_flat", max_order=127)
    refused("orders up to 128", check_ragged_call, CPU, plan_of([4, 129]), torch.float32)


# ---- the pointer calls ------------------------------------------------------------------------------------------------
def test_element_type():
    for dtype in (torch.float16, torch.bfloat16, torch.int32, None):
        refused("dtype: expected torch.float32 or torch.float64", pointer_args, dtype=dtype)
    refused("dtype: expected torch.float32 or torch.float64", check_packed_matrices, CPU, PLAN,
            torch.zeros(FLAT, dtype=torch.float16), "a_flat")
    refused("the matrix: expected torch.float32 or torch.float64", check_diag_blocks, CPU,
            torch.zeros(ROWS, ROWS, dtype=torch.float16), ORDERS)
    for dtype in (torch.float32, torch.float64):
        pointer_args(dtype=dtype)
        check_packed_matrices(CPU, PLAN, torch.zeros(FLAT, dtype=dtype), "a_flat")
        check_diag_blocks(CPU, torch.zeros(ROWS, ROWS, dtype=dtype), ORDERS)


@pytest.mark.parametrize("nrhs", [0, -2, 2.5])
def test_nrhs_refusals(nrhs):
    refused("nrhs: at least one column", pointer_args, nrhs=nrhs)


def test_nrhs_accepted():
    pointer_args(nrhs=1)
    pointer_args(nrhs=7)
    pointer_args(nrhs=np.int64(3))


def test_pointer_tensor_refusals():
    good = ptrs()
    for name in ("a_ptrs", "b_ptrs", "x_ptrs"):
        def call(bad):
            return pointer_args(p=dict({"a_ptrs": good, "b_ptrs": good, "x_ptrs": good}, **{name: bad}), nrhs=1)
        refused(f"{name} is torch.int32", call, ptrs(dtype=torch.int32))
        refused(f"{name} is torch.float64", call, ptrs(dtype=torch.float64))
        refused(f"{name} is on meta", call, ptrs(device="meta"))
        refused(f"{name}: expected a contiguous 1-D tensor of 3 entries", call, ptrs(2))
        refused(f"{name}: expected a contiguous 1-D tensor of 3 entries", call, ptrs(4))
        refused(f"{name}: expected a contiguous 1-D", call, ptrs(6)[::2])
        refused(f"{name}: expected a contiguous 1-D", call, ptrs().view(3, 1))


def test_leading_dimension_refusals():
    for name in ("lda", "ldout"):
        def call(bad):
            return pointer_args(lds={"lda": None, "ldout": None, name: bad})
        refused(f"{name} is torch.int64", call, ptrs())
        refused(f"{name} is on meta", call, ptrs(dtype=torch.int32, device="meta"))
        refused(f"{name}: expected a contiguous 1-D tensor of 3 entries", call, ptrs(2, torch.int32))
        refused(f"{name}: expected a contiguous 1-D", call, ptrs(6, torch.int32)[::2])
        call(ptrs(dtype=torch.int32))
        call(None)


def test_status_refusals():
    refused("status is torch.int64", pointer_args, status=ptrs())
    refused("status is torch.float32", pointer_args, status=torch.zeros(BATCH))
    refused("status is on meta", pointer_args, status=ptrs(dtype=torch.int32, device="meta"))
    refused("status: expected a contiguous 1-D tensor of 3 entries", pointer_args, status=ptrs(2, torch.int32))
    refused("of 3 entries", pointer_args, status=ptrs(4, torch.int32))
    refused("contiguous 1-D", pointer_args, status=ptrs(6, torch.int32)[::2])
    refused("contiguous 1-D", pointer_args, status=ptrs(dtype=torch.int32).view(3, 1))


def test_status_is_allocated_or_returned():
    st = pointer_args()
    assert st.dtype == torch.int32 and st.shape == (BATCH,) and st.device == CPU and st.is_contiguous()
    given = ptrs(dtype=torch.int32)
    assert pointer_args(status=given) is given
    assert pointer_args(nrhs=2, want_status=False) is None                                       # apply has none
    # the packed calls hand theirs through the same check
    st = check_packed_matrices(CPU, PLAN, torch.zeros(FLAT), "a_flat")
    assert st.dtype == torch.int32 and st.shape == (BATCH,)
    assert check_packed_matrices(CPU, PLAN, torch.zeros(FLAT), "a_flat", given) is given
    assert check_packed_matrices(CPU, PLAN, torch.zeros(FLAT), "x_flat", want_status=False) is None
    refused("status is torch.int64", check_packed_matrices, CPU, PLAN, torch.zeros(FLAT), "a_flat", ptrs())


# ---- the packed matrices ----------------------------------------------------------------------------------------------
def test_packed_matrix_refusals():
    def call(flat):
        return check_packed_matrices(CPU, PLAN, flat, "a_flat")
    refused("a_flat: expected a contiguous 1-D tensor of 4997 entries", call, torch.zeros(FLAT - 1))
    refused("of 4997 entries", call, torch.zeros(FLAT + 1))
    refused("a_flat: expected a contiguous 1-D", call, torch.zeros(2 * FLAT)[::2])
    refused("a_flat: expected a contiguous 1-D", call, torch.zeros(FLAT, 1))
    refused("a_flat is on meta", call, torch.zeros(FLAT, device="meta"))
    call(torch.zeros(FLAT))
    call(torch.zeros(FLAT + 1, dtype=torch.float64)[1:])                                         # element alignment is enough


# ---- the packed right-hand side ---------------------------------------------------------------------------------------
def test_packed_rhs_refusals():
    a = torch.zeros(FLAT)

    def call(b, out=None):
        return check_packed_rhs(PLAN, a, b, out, "b")
    refused("b is torch.float64 on cpu, expected torch.float32", call, torch.zeros(ROWS, K, dtype=torch.float64))
    refused("b is torch.float32 on meta", call, torch.zeros(ROWS, K, device="meta"))
    refused(r"b: expected \(83,\) or \(83, K\)", call, torch.zeros(ROWS - 1, K))
    refused(r"b: expected \(83,\) or \(83, K\)", call, torch.zeros(ROWS, K, 2))
    refused(r"b: expected \(83,\) or \(83, K\)", call, torch.zeros(ROWS, 0))
    refused(r"b: expected \(83,\) or \(83, K\)", call, torch.zeros(()))
    b = torch.zeros(ROWS, K)
    refused("out: b itself or a contiguous tensor of its shape", call, b, torch.zeros(ROWS, K + 1))
    refused("out: b itself or a contiguous tensor of its shape", call, b, torch.zeros(ROWS))
    refused("out: b itself or a contiguous tensor of its shape", call, b, torch.zeros(ROWS, K, dtype=torch.float64))
    refused("out: b itself or a contiguous tensor of its shape", call, b, torch.zeros(ROWS, K, device="meta"))
    refused("out: b itself or a contiguous tensor of its shape", call, b, torch.zeros(K, ROWS).t())
    refused("out: b itself or a contiguous tensor of its shape", call, b, a)                     # out is a_flat


def test_packed_rhs_accepted_forms():
    a = torch.zeros(FLAT, dtype=torch.float64)
    vec, b = torch.zeros(ROWS, dtype=torch.float64), torch.zeros(ROWS, K, dtype=torch.float64)
    rhs, out, nrhs = check_packed_rhs(PLAN, a, vec, None, "b")
    assert nrhs == 1 and rhs is vec and out.shape == (ROWS,) and out.dtype == torch.float64 and out.is_contiguous()
    assert out.data_ptr() != vec.data_ptr()
    rhs, out, nrhs = check_packed_rhs(PLAN, a, b, None, "b")
    assert nrhs == K and rhs is b and out.shape == (ROWS, K)
    rhs, out, nrhs = check_packed_rhs(PLAN, a, b, b, "b")                                         # in place
    assert nrhs == K and rhs is out and out is b
    other = torch.empty(ROWS, K, dtype=torch.float64)
    rhs, out, nrhs = check_packed_rhs(PLAN, a, b, other, "b")
    assert rhs is b and out is other
    bt = torch.zeros(K, ROWS, dtype=torch.float64).t()                                            # a non-contiguous b is copied
    rhs, out, nrhs = check_packed_rhs(PLAN, a, bt, None, "b")
    assert rhs.is_contiguous() and rhs.shape == (ROWS, K) and nrhs == K
    check_packed_rhs(PLAN, a, a[:ROWS * K].view(ROWS, K), None, "b")                              # b in a_flat: both are read


# ---- the aliasing rule ------------------------------------------------------------------------------------------------
def test_out_over_the_matrices_is_refused():
    """``solve_ragged`` and ``apply_ragged``: anywhere in a_flat, not only at its start."""
    a, b = torch.zeros(FLAT), torch.zeros(ROWS)
    refused("out must not alias the matrices", check_packed_rhs, PLAN, a, b, a[2:2 + ROWS], "b")
    refused("out must not alias the matrices", check_packed_rhs, PLAN, a, b, a[:ROWS], "b")
    refused("out must not alias the matrices", check_packed_rhs, PLAN, a, b, a[FLAT - ROWS:], "b")
    inside = a[:ROWS]
    refused("out must not alias the matrices", check_packed_rhs, PLAN, a, inside, inside, "b")   # in place, but inside a_flat
    buf = torch.zeros(FLAT + ROWS)
    refused("out must not alias the matrices", check_packed_rhs, PLAN, buf[:FLAT], b, buf[FLAT - 1:-1], "b")
    check_packed_rhs(PLAN, buf[:FLAT], b, buf[FLAT:], "b")                                        # the neighbour is fine
    assert check_packed_rhs(PLAN, a, b, b, "b")[0] is b                                           # out is b: accepted


def test_out_over_a_part_of_the_right_hand_side_is_refused():
    a, buf = torch.zeros(FLAT), torch.zeros(2 * ROWS)
    b = buf[:ROWS]
    refused("not a part of its memory", check_packed_rhs, PLAN, a, b, buf[2:2 + ROWS], "b")
    refused("not a part of its memory", check_packed_rhs, PLAN, a, b, buf[ROWS - 1:2 * ROWS - 1], "b")
    refused("not a part of its memory", check_packed_rhs, PLAN, a, buf[1:ROWS + 1], b, "b")
    check_packed_rhs(PLAN, a, b, buf[ROWS:], "b")
    rhs, out, _ = check_packed_rhs(PLAN, a, b, buf[:ROWS], "b")                                  # another tensor over b's memory
    assert rhs.data_ptr() == out.data_ptr() == b.data_ptr()


def test_solve_diag_blocks_out_over_the_matrix_is_refused():
    """``solve_diag_blocks`` and ``apply_diag_blocks``: the matrix stands where a_flat does."""
    m, r = torch.zeros(ROWS, ROWS), torch.zeros(ROWS)
    refused("out must not alias the matrices", check_packed_rhs, PLAN, m, r, m[1], "r")
    refused("out must not alias the matrices", check_packed_rhs, PLAN, m, r, m.view(-1)[2:2 + ROWS], "r")
    assert check_packed_rhs(PLAN, m, r, r, "r")[0] is r


def test_inverse_out_in_place_or_apart():
    """``inv_ragged`` / ``inv_diag_blocks``: the input itself or memory apart from it, never a partial overlap."""
    buf = torch.zeros(2 * FLAT)
    a = buf[:FLAT]
    assert check_inverse_out(a, a, a.shape) is a                                                  # in place
    assert check_inverse_out(a, buf[:FLAT], a.shape).data_ptr() == a.data_ptr()
    refused("not a part of its memory", check_inverse_out, a, buf[2:FLAT + 2], a.shape)
    refused("not a part of its memory", check_inverse_out, a, buf[FLAT - 1:2 * FLAT - 1], a.shape)
    assert check_inverse_out(a, buf[FLAT:], a.shape).data_ptr() == buf.data_ptr() + 4 * FLAT
    out = check_inverse_out(a, None, a.shape)
    assert out.shape == (FLAT,) and out.dtype == a.dtype and out.data_ptr() != a.data_ptr()
    # the dense matrix of inv_diag_blocks: zeros where none is given, in place or apart
    mbuf = torch.ones(2 * ROWS * ROWS)
    m = mbuf[:ROWS * ROWS].view(ROWS, ROWS)
    assert check_inverse_out(m, m, m.shape, zero=True) is m
    refused("not a part of its memory", check_inverse_out, m, mbuf[2:ROWS * ROWS + 2].view(ROWS, ROWS), m.shape, zero=True)
    z = check_inverse_out(m, None, m.shape, zero=True)
    assert z.shape == m.shape and not z.any()
    # packed=True: the packed output beside the dense input
    refused("not a part of its memory", check_inverse_out, m, mbuf[2:FLAT + 2], (FLAT,))
    refused("not a part of its memory", check_inverse_out, m, mbuf[:FLAT], (FLAT,))               # same start, other extent
    assert check_inverse_out(m, mbuf[ROWS * ROWS:ROWS * ROWS + FLAT], (FLAT,)).shape == (FLAT,)


def test_inverse_out_refusals():
    a = torch.zeros(FLAT)
    refused("out: a contiguous tensor of shape", check_inverse_out, a, torch.zeros(FLAT, dtype=torch.float64), a.shape)
    refused("out: a contiguous tensor of shape", check_inverse_out, a, torch.zeros(FLAT, device="meta"), a.shape)
    refused("out: a contiguous tensor of shape", check_inverse_out, a, torch.zeros(FLAT - 1), a.shape)
    refused("out: a contiguous tensor of shape", check_inverse_out, a, torch.zeros(2 * FLAT)[::2], a.shape)
    m = torch.zeros(ROWS, ROWS)
    refused("out: a contiguous tensor of shape", check_inverse_out, m, torch.zeros(ROWS, ROWS).t(), m.shape)
    refused("out: a contiguous tensor of shape", check_inverse_out, m, torch.zeros(ROWS * ROWS), m.shape)


# ---- the dense diagonal-block matrix ----------------------------------------------------------------------------------
def test_diag_block_refusals():
    m = torch.zeros(ROWS, ROWS)
    refused("block_orders must sum to the matrix order", check_diag_blocks, CPU, m, [4, 9, 69])
    refused("block_orders must sum to the matrix order", check_diag_blocks, CPU, torch.zeros(5, 5), [2, 2])
    refused("block_orders: a non-empty 1-D sequence", check_diag_blocks, CPU, m, [])
    refused("block_orders: a non-empty 1-D sequence", check_diag_blocks, CPU, m, [[4, 9, 70]])
    refused("expected a contiguous square matrix", check_diag_blocks, CPU, torch.zeros(ROWS, ROWS + 1), ORDERS)
    refused("expected a contiguous square matrix", check_diag_blocks, CPU, torch.zeros(ROWS * ROWS), ORDERS)
    refused("expected a contiguous square matrix", check_diag_blocks, CPU, torch.zeros(ROWS, 2 * ROWS)[:, ::2], ORDERS)
    refused("the matrix is on meta", check_diag_blocks, CPU, torch.zeros(ROWS, ROWS, device="meta"), ORDERS)
    assert check_diag_blocks(CPU, m, ORDERS).tolist() == ORDERS
    assert check_diag_blocks(CPU, m, np.array(ORDERS)).tolist() == ORDERS
    assert check_diag_blocks(CPU, None, [4, 9]).tolist() == [4, 9]                                # packed: any sum
    refused("block_orders: a non-empty 1-D sequence", check_diag_blocks, CPU, None, [])
