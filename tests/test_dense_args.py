"""Host-only tests of ``api.check_dense_args``, the argument check behind ``Inverter.inv`` / ``inv_det`` /
``inv_det_any`` / ``solve``: one test per refusal and one per accepted form, on CPU tensors with
``device=torch.device("cpu")`` standing for the Inverter's device and ``device="meta"`` tensors standing for "on another
device".  No handle, no library, no GPU.  tests/test_gpu_memory_contract.py repeats every refusal through a live
``Inverter``."""
import pytest
import torch

from gpu_matrix_inversion_amd.api import check_dense_args

CPU = torch.device("cpu")
B, N, K = 3, 4, 2


def mats(dtype=torch.float32, batch=B, n=N):
    return torch.arange(batch * n * n, dtype=dtype).reshape(batch, n, n)


def rhs(dtype=torch.float32, batch=B, n=N, k=K):
    return torch.arange(batch * n * k, dtype=dtype).reshape(batch, n, k)


def refused(match, *args, **kw):
    with pytest.raises(ValueError, match=match):
        check_dense_args(CPU, *args, **kw)


# ---- refusals: a ------------------------------------------------------------------------------------------------------
def test_a_on_another_device_is_refused():
    refused("expected a float32 or float64 tensor on the GPU", torch.empty(B, N, N, device="meta"))
    refused("on the GPU", torch.empty(B, N, N, device="meta"), b=torch.empty(B, N, K, device="meta"))


def test_a_of_another_dtype_or_shape_is_refused():
    refused("float32 or float64", mats(torch.float16))
    refused(r"\(N,N\) or \(B,N,N\)", torch.zeros(B, N, N + 1))
    refused(r"\(N,N\) or \(B,N,N\)", torch.zeros(0, N, N))
    refused("inv_det takes orders up to 128", torch.zeros(1, 129, 129), max_order=128)
    refused("solve takes orders up to 127", torch.zeros(1, 128, 128), b=torch.zeros(1, 128, 1))


# ---- refusals: out ----------------------------------------------------------------------------------------------------
def test_out_of_another_dtype_is_refused():
    refused("out is torch.float64", mats(), out=torch.empty(B, N, N, dtype=torch.float64))
    refused("out is torch.float32", mats(torch.float64), out=torch.empty(B, N, N))
    # the case of the report: an fp64 buffer of half the elements has the bytes, and used to come back half written
    refused("out is torch.float64", mats(), out=torch.empty(B * N * N // 2, dtype=torch.float64))


def test_out_on_another_device_is_refused():
    refused("out is torch.float32 on meta", mats(), out=torch.empty(B, N, N, device="meta"))


def test_out_of_a_wrong_element_count_is_refused():
    refused("out holds", mats(), out=torch.empty(B, N, N + 1))
    refused("out holds", mats(), out=torch.empty(B * N * N - 1))
    refused("out holds", mats()[0], out=torch.empty(B, N, N))


def test_out_not_contiguous_is_refused():
    refused("out must be contiguous", mats(), out=torch.empty(B, N, N).transpose(1, 2))
    refused("out must be contiguous", mats(), out=torch.empty(B, N, 2 * N)[:, :, ::2])
    refused("out must be contiguous", mats(), out=torch.empty(2 * B * N * N)[::2])   # used to be view()'s RuntimeError


def test_out_overlapping_a_anywhere_is_refused():
    buf = torch.zeros(2 * B * N * N)
    size = B * N * N
    a = buf[:size].view(B, N, N)
    refused("must not alias the input", a, out=a)                                  # the same start: refused before
    refused("must not alias the input", a, out=buf[1:size + 1])                    # one element later
    refused("must not alias the input", a, out=buf[size - 1:2 * size - 1])         # its first element is a's last
    back = buf[size:].view(B, N, N)
    refused("must not alias the input", back, out=buf[1:size + 1])                 # its last element is a's first
    check_dense_args(CPU, a, out=buf[size:])                                       # the neighbour is fine


def test_out_with_want_inverse_false_is_refused():
    refused("want_inverse=False", mats(), out=torch.empty(B, N, N), want_inverse=False)


# ---- refusals: status -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solve", [False, True], ids=["inv", "solve"])
def test_status_refusals(solve):
    kw = {"b": rhs()} if solve else {}
    refused("status is torch.int64", mats(), status=torch.zeros(B, dtype=torch.int64), **kw)
    refused("status is torch.float32", mats(), status=torch.zeros(B), **kw)
    refused("status is on meta", mats(), status=torch.zeros(B, dtype=torch.int32, device="meta"), **kw)
    refused("status: expected a contiguous 1-D tensor of 3 entries", mats(), status=torch.zeros(B - 1, dtype=torch.int32),
            **kw)                                                                  # short: used to be written past its end
    refused("of 3 entries", mats(), status=torch.zeros(B + 1, dtype=torch.int32), **kw)
    refused("contiguous 1-D", mats(), status=torch.zeros(2 * B, dtype=torch.int32)[::2], **kw)
    refused("contiguous 1-D", mats(), status=torch.zeros(B, 1, dtype=torch.int32), **kw)
    refused("of 1 entries", mats()[0], status=torch.zeros(B, dtype=torch.int32), **({"b": rhs()[0]} if solve else {}))


# ---- refusals: solve --------------------------------------------------------------------------------------------------
def test_solve_b_refusals():
    refused("b is torch.float64", mats(), b=rhs(torch.float64))
    refused("b is torch.float32 on meta", mats(), b=torch.empty(B, N, K, device="meta"))
    refused("b: expected a's batch dimension", mats(), b=torch.zeros(B, N + 1, K))
    refused("b: expected a's batch dimension", mats(), b=torch.zeros(B + 1, N, K))


def test_solve_out_refusals():
    a, b = mats(), rhs()
    refused("out is torch.float64", a, out=torch.empty(B, N, K, dtype=torch.float64), b=b)
    refused("out is torch.float32 on meta", a, out=torch.empty(B, N, K, device="meta"), b=b)
    refused("out: b itself or a contiguous tensor of b's shape", a, out=torch.empty(B, K, N), b=b)
    refused("out: b itself or a contiguous tensor of b's shape", a, out=torch.empty(B, K, N).transpose(1, 2), b=b)
    refused("out: b itself or a contiguous tensor of b's shape", a, out=torch.empty(B * N * K), b=b)


def test_solve_out_overlapping_a_is_refused():
    buf = torch.zeros(B * N * N + B * N * K)
    a = buf[:B * N * N].view(B, N, N)
    b = rhs()
    refused("out must not alias a", a, out=buf[:B * N * K].view(B, N, K), b=b)     # the same start: refused before
    refused("out must not alias a", a, out=buf[5:5 + B * N * K].view(B, N, K), b=b)
    refused("out must not alias a", a, out=buf[B * N * N - 1:-1].view(B, N, K), b=b)
    check_dense_args(CPU, a, out=buf[B * N * N:].view(B, N, K), b=b)


def test_solve_out_partly_over_b_is_refused():
    buf = torch.zeros(2 * B * N * K)
    size = B * N * K
    b = buf[:size].view(B, N, K)
    a = mats()
    refused("not a part of b's memory", a, out=buf[1:size + 1].view(B, N, K), b=b)
    refused("not a part of b's memory", a, out=buf[size - 1:2 * size - 1].view(B, N, K), b=b)
    refused("not a part of b's memory", a, out=b, b=buf[size - 1:2 * size - 1].view(B, N, K))
    check_dense_args(CPU, a, out=buf[size:].view(B, N, K), b=b)


# ---- accepted forms ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_batch_without_out_and_status(dtype):
    a = mats(dtype)
    squeeze, a3, r, out, status = check_dense_args(CPU, a)
    assert not squeeze and r is None and a3.data_ptr() == a.data_ptr() and a3.shape == (B, N, N)
    assert out.shape == (B, N, N) and out.dtype == dtype and out.is_contiguous() and out.data_ptr() != a.data_ptr()
    assert status.shape == (B,) and status.dtype == torch.int32 and status.device == CPU


def test_single_matrix_squeezes():
    a = mats()[1]
    squeeze, a3, _, out, status = check_dense_args(CPU, a)
    assert squeeze and a3.shape == (1, N, N) and a3.data_ptr() == a.data_ptr() and out.shape == (1, N, N)
    assert status.shape == (1,)


def test_given_out_and_status_are_the_ones_returned():
    a, out, st = mats(), torch.empty(B, N, N), torch.empty(B, dtype=torch.int32)
    _, _, _, out3, status = check_dense_args(CPU, a, out, st)
    assert status is st and out3.data_ptr() == out.data_ptr() and out3.shape == (B, N, N)


def test_out_of_any_shape_with_the_element_count_is_viewed():
    for shape in ((B * N * N,), (1, B * N * N), (B * N, N)):
        out = torch.empty(shape)
        assert check_dense_args(CPU, mats(), out)[3].data_ptr() == out.data_ptr()
    out = torch.empty(N * N)
    assert check_dense_args(CPU, mats()[0], out)[3].shape == (1, N, N)


def test_element_aligned_views_are_accepted():
    """A view one element into its buffer is contiguous: element alignment is all the dense calls ask for."""
    buf_a, buf_o, buf_s = torch.zeros(B * N * N + 1), torch.zeros(B * N * N + 1), torch.zeros(B + 1, dtype=torch.int32)
    a, out, st = buf_a[1:].view(B, N, N), buf_o[1:], buf_s[1:]
    _, a3, _, out3, status = check_dense_args(CPU, a, out, st)
    assert a3.data_ptr() == buf_a.data_ptr() + 4 and out3.data_ptr() == buf_o.data_ptr() + 4
    assert status.data_ptr() == buf_s.data_ptr() + 4


@pytest.mark.parametrize("view", ["transposed", "every_other", "expanded"])
def test_non_contiguous_a_is_copied(view):
    base = torch.arange(2 * B * N * N, dtype=torch.float32).reshape(2 * B, N, N)
    a = {"transposed": base[:B].transpose(1, 2), "every_other": base[::2], "expanded": base[0].expand(B, N, N)}[view]
    assert not a.is_contiguous()
    _, a3, _, out, _ = check_dense_args(CPU, a)
    assert a3.is_contiguous() and torch.equal(a3, a) and out.shape == (B, N, N)
    ptrs = {a3.data_ptr() + 4 * i for i in (0, a3.numel() - 1)}
    assert not any(base.data_ptr() <= p < base.data_ptr() + 4 * base.numel() for p in ptrs)
    # out may then be the memory the view was taken from: the copy is what is read
    check_dense_args(CPU, base[:B].transpose(1, 2), out=base[:B])


def test_want_inverse_false_gives_no_out():
    _, a3, _, out, status = check_dense_args(CPU, mats(), want_inverse=False, max_order=128)
    assert out is None and status.shape == (B,) and a3.shape == (B, N, N)


def test_max_order_is_accepted_at_the_limit():
    check_dense_args(CPU, torch.zeros(1, 128, 128), max_order=128)
    check_dense_args(CPU, torch.zeros(1, 129, 129))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_solve_forms(dtype):
    a, b = mats(dtype), rhs(dtype)
    squeeze, a3, r, out3, status = check_dense_args(CPU, a, b=b)
    assert not squeeze and r.data_ptr() == b.data_ptr() and out3.shape == (B, N, K) and out3.dtype == dtype
    assert out3.data_ptr() != b.data_ptr() and status.shape == (B,)
    # a vector per member keeps one column
    vec = b[:, :, 0].contiguous()
    _, _, r, out3, _ = check_dense_args(CPU, a, b=vec)
    assert r.shape == (B, N, 1) and out3.shape == (B, N, 1)
    # a single system
    squeeze, a3, r, out3, status = check_dense_args(CPU, a[0], b=b[0])
    assert squeeze and a3.shape == (1, N, N) and r.shape == (1, N, K) and out3.shape == (1, N, K) and status.shape == (1,)
    _, _, r, out3, _ = check_dense_args(CPU, a[0], b=vec[0])
    assert r.shape == (1, N, 1) and out3.shape == (1, N, 1)
    # a separate out
    out = torch.empty(B, N, K, dtype=dtype)
    _, _, r, out3, _ = check_dense_args(CPU, a, out=out, b=b)
    assert out3.data_ptr() == out.data_ptr() and r.data_ptr() == b.data_ptr()
    # a non-contiguous b is copied
    bt = torch.zeros(B, K, N, dtype=dtype).transpose(1, 2)
    _, _, r, _, _ = check_dense_args(CPU, a, b=bt)
    assert r.is_contiguous() and r.shape == (B, N, K)


def test_solve_in_place_is_the_one_alias():
    a, b = mats(), rhs()
    _, _, r, out3, _ = check_dense_args(CPU, a, out=b, b=b)
    assert r.data_ptr() == out3.data_ptr() == b.data_ptr()
    # another tensor object over exactly b's memory is the same call
    _, _, r, out3, _ = check_dense_args(CPU, a, out=b.view(B, N, K), b=b)
    assert r.data_ptr() == out3.data_ptr() == b.data_ptr()
    # b may share memory with a: both are only read
    buf = torch.zeros(B * N * N)
    check_dense_args(CPU, buf.view(B, N, N), b=buf[:B * N * K].view(B, N, K))
