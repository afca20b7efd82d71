"""Host-only tests of the argument handling behind ``Inverter.csr_diag_blocks`` / ``inv_csr_blocks``: ``api.csr_parts``,
``check_csr``, ``check_csr_first_rows``, ``check_csr_out`` and ``validate_csr``.  One assertion per refusal and the
accepted form beside it, on CPU tensors with ``device=torch.device("cpu")`` standing for the Inverter's device and
``device="meta"`` tensors for "on another device", as tests/test_ragged_args.py does.  No handle, no library, no GPU."""
import inspect

import numpy as np
import pytest
import torch

import gpu_matrix_inversion_amd as g
from gpu_matrix_inversion_amd.api import check_csr, check_csr_first_rows, check_csr_out, csr_parts, validate_csr

CPU = torch.device("cpu")
N, NNZ = 5, 7


def refused(match, fn, *args, **kw):
    with pytest.raises(ValueError, match=match):
        fn(*args, **kw)


def triple(idtype=torch.int64, vdtype=torch.float32, **kw):
    """A 5 x 5 matrix of 7 entries; row 1 is empty and row 3 unsorted."""
    return (torch.tensor([0, 2, 2, 3, 6, 7], dtype=idtype, **kw), torch.tensor([0, 4, 2, 3, 0, 1, 4], dtype=idtype, **kw),
            torch.arange(1, NNZ + 1, dtype=vdtype, **kw))


def test_signatures():
    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert sig(g.Inverter.csr_diag_blocks) == ["self", "a", "block_orders", "out", "first_rows", "validate"]
    assert sig(g.Inverter.inv_csr_blocks) == ["self", "a", "block_orders", "first_rows", "det", "validate"]
    for f in (g.Inverter.csr_diag_blocks, g.Inverter.inv_csr_blocks):
        p = inspect.signature(f).parameters
        assert p["first_rows"].kind is p["validate"].kind is inspect.Parameter.KEYWORD_ONLY
        assert p["first_rows"].default is None and p["validate"].default is False


# ---- one argument form ------------------------------------------------------------------------------------------------
def test_csr_tensor_or_triple():
    crow, col, val = triple()
    a = torch.sparse_csr_tensor(crow, col, val, size=(N, N))
    parts = csr_parts(a)
    assert all(torch.equal(p, q) for p, q in zip(parts, (crow, col, val)))
    assert check_csr(CPU, *parts) == N
    assert csr_parts((crow, col, val)) == (crow, col, val) and csr_parts([crow, col, val]) == (crow, col, val)
    batched = torch.sparse_csr_tensor(torch.stack((crow, crow)), torch.stack((col, col)), torch.stack((val, val)),
                                      size=(2, N, N))
    refused("batched CSR tensors are not taken", csr_parts, batched)
    refused("expected a square matrix", csr_parts, torch.sparse_csr_tensor(crow, col, val, size=(N, N + 1)))
    refused("expected a torch.sparse_csr tensor or a", csr_parts, a.to_dense())
    refused("expected a torch.sparse_csr tensor or a", csr_parts, a.to_sparse_coo())
    refused("expected a torch.sparse_csr tensor or a", csr_parts, (crow, col))
    refused("expected a torch.sparse_csr tensor or a", csr_parts, (crow, col, val.numpy()))
    refused("expected a torch.sparse_csr tensor or a", csr_parts, None)


# ---- check_csr ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("vdtype", [torch.float32, torch.float64])
def test_accepted_dtypes(idtype, vdtype):
    assert check_csr(CPU, *triple(idtype, vdtype)) == N


def test_dtype_refusals():
    crow, col, val = triple()
    refused("crow is torch.int16", check_csr, CPU, crow.short(), col.short(), val)
    refused("crow is torch.float32", check_csr, CPU, crow.float(), col, val)
    refused("col is torch.int32, crow torch.int64: expected one index dtype", check_csr, CPU, crow, col.int(), val)
    refused("col is torch.int64, crow torch.int32", check_csr, CPU, crow.int(), col, val)
    refused("values: expected torch.float32 or torch.float64", check_csr, CPU, crow, col, val.half())
    refused("values: expected torch.float32 or torch.float64", check_csr, CPU, crow, col, val.long())


def test_layout_and_count_refusals():
    crow, col, val = triple()
    wide = torch.zeros(2 * NNZ, dtype=torch.int64)
    refused("col: expected a contiguous 1-D", check_csr, CPU, crow, wide[::2], val)
    refused("crow: expected a contiguous 1-D", check_csr, CPU, torch.zeros(2 * N + 2, dtype=torch.int64)[::2], col, val)
    refused("values: expected a contiguous 1-D", check_csr, CPU, crow, col, torch.zeros(2 * NNZ)[::2])
    refused("values: expected a contiguous 1-D", check_csr, CPU, crow, col, val.view(NNZ, 1))
    refused("crow: expected a contiguous 1-D", check_csr, CPU, crow.view(1, -1), col, val)
    refused("values holds 6 entries, col 7", check_csr, CPU, crow, col, val[:-1])
    refused("values holds 7 entries, col 6", check_csr, CPU, crow, col[:-1], val)
    refused("crow: at least 2 entries", check_csr, CPU, crow[:1], col, val)
    assert check_csr(CPU, crow[:2], col, val) == 1                    # what the arrays hold is validate's business
    assert check_csr(CPU, crow, col[1:], val[1:]) == N                # element alignment is enough


def test_device_refusals():
    crow, col, val = triple()
    mcrow, mcol, mval = triple(device="meta")
    refused("crow is on meta", check_csr, CPU, mcrow, col, val)
    refused("col is on meta", check_csr, CPU, crow, mcol, val)
    refused("values is on meta", check_csr, CPU, crow, col, mval)
    refused("crow is on cpu, expected meta", check_csr, torch.device("meta"), crow, col, val)
    assert check_csr(torch.device("meta"), mcrow, mcol, mval) == N


# ---- first_rows --------------------------------------------------------------------------------------------------------
def test_first_rows_rule():
    assert check_csr_first_rows(None, [2, 3], N).tolist() == [0, 2]
    refused("block_orders sum to 4, the matrix has 5 rows", check_csr_first_rows, None, [2, 2], N)
    refused("block_orders sum to 6", check_csr_first_rows, None, [3, 3], N)
    f = check_csr_first_rows([3, 0, 0], [2, 2, 5], N)                 # overlapping blocks, any order, any sum
    assert f.dtype == np.int64 and f.tolist() == [3, 0, 0]
    assert check_csr_first_rows(np.array([1], np.int32), [2], N).tolist() == [1]     # a gap on either side
    refused("first_rows: block 1 .rows 4 ... 5. leaves the matrix of 5 rows", check_csr_first_rows, [0, 4], [2, 2], N)
    refused("first_rows: block 0 .rows -1 ... 0. leaves the matrix", check_csr_first_rows, [-1, 2], [2, 2], N)
    refused("first_rows: a 1-D integer sequence of 2 entries", check_csr_first_rows, [0], [2, 2], N)
    refused("first_rows: a 1-D integer sequence of 2 entries", check_csr_first_rows, [0, 1, 2], [2, 2], N)
    refused("first_rows: a 1-D integer sequence of 2 entries", check_csr_first_rows, [[0, 2]], [2, 2], N)
    refused("first_rows: a 1-D integer sequence of 2 entries", check_csr_first_rows, [0.0, 2.0], [2, 2], N)


# ---- out ---------------------------------------------------------------------------------------------------------------
def test_out_rule():
    val = torch.zeros(NNZ + 13)[:NNZ]
    out = check_csr_out(val, None, 13)
    assert out.shape == (13,) and out.dtype == val.dtype and out.is_contiguous() and out.data_ptr() != val.data_ptr()
    given = torch.empty(13)
    assert check_csr_out(val, given, 13) is given
    refused("out: expected a contiguous 1-D tensor of 13 entries", check_csr_out, val, torch.empty(12), 13)
    refused("out: expected a contiguous 1-D tensor of 13 entries", check_csr_out, val, torch.empty(26)[::2], 13)
    refused("out: expected a contiguous 1-D tensor of 13 entries", check_csr_out, val, torch.empty(13, 1), 13)
    refused("out is torch.float64, expected torch.float32", check_csr_out, val, torch.empty(13, dtype=torch.float64), 13)
    refused("out is on meta", check_csr_out, val, torch.empty(13, device="meta"), 13)
    buf = torch.zeros(NNZ + 13)
    refused("out must not alias values", check_csr_out, buf[:NNZ], buf[NNZ - 1:NNZ + 12], 13)      # one element shared
    refused("out must not alias values", check_csr_out, buf[2:2 + NNZ], buf[:13], 13)
    assert check_csr_out(buf[:NNZ], buf[NNZ:], 13).data_ptr() == buf.data_ptr() + 4 * NNZ          # the neighbour is fine


# ---- validate=True -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
def test_validate(idtype):
    crow, col, _ = triple(idtype)
    validate_csr(crow, col, N)
    validate_csr(torch.zeros(N + 1, dtype=idtype), col[:0], N)        # an empty matrix
    bad = crow.clone()
    bad[0] = 1
    refused("crow.0. is 1, expected 0", validate_csr, bad, col, N)
    bad = crow.clone()
    bad[-1] = NNZ - 1
    refused("crow.-1. is 6, expected the 7 entries of col", validate_csr, bad, col, N)
    bad = crow.clone()
    bad[2] = 1                                                        # 0 2 1 3 6 7
    refused("crow decreases", validate_csr, bad, col, N)
    bad = col.clone()
    bad[3] = N                                                        # a column equal to N
    refused("col: expected 0 <= col < 5", validate_csr, crow, bad, N)
    bad = col.clone()
    bad[0] = -1
    refused("col: expected 0 <= col < 5", validate_csr, crow, bad, N)
    bad = col.clone()
    bad[5] = 3                                                        # row 3: 3 3 1
    refused(r"entry \(3, 3\) is stored twice", validate_csr, crow, bad, N)
    same_col_other_row = col.clone()
    same_col_other_row[2] = 0                                         # (2, 0) beside (0, 0) and (3, 0): no duplicate
    validate_csr(crow, same_col_other_row, N)
