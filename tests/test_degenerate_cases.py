"""CPU-only proof that the inputs of tests/degenerate_cases.py are what they claim to be: the oracle gives the stated
status in every one of its forms, fp32 and fp64, and for the exact families its inverse equals the inverse the
generator wrote down (bytes, -0.0 stored as +0.0).  A precondition of tests/test_gpu_degenerate.py, not a measurement:
no tolerance anywhere."""
import collections

import numpy as np
import pytest

from conftest import canonical_bytes, gate_matrix
from degenerate_cases import (OVERFLOW_LIST, STATUS_OK, STATUS_SINGULAR, block_diagonal, canon, duplicate_rows,
                              exact_families, ones_block, overflow, place_blocks, zero_column, zero_row)

ORDERS = [1, 2, 3, 5, 17, 64, 65, 130, 257, 300]


def oracle_forms(oracle, dtype):
    """{name: fn(a, n) -> (flat inverse, status)} of every form of the oracle for this dtype."""
    def wrap(fn, *extra):
        def call(a, n):
            x, info = fn(a, n, *extra, return_info=True)
            return x, int(info["status"])
        return call
    if np.dtype(dtype) == np.float32:
        return {"augmented": wrap(oracle.matrix_inv_32), "inplace": wrap(oracle.matrix_inv_32_inplace),
                "blocked_exact64": wrap(oracle.matrix_inv_32_blocked_exact, 64),
                "blocked_exact128": wrap(oracle.matrix_inv_32_blocked_exact, 128)}
    return {"inplace64": wrap(oracle.matrix_inv_64), "blocked64_64": wrap(oracle.matrix_inv_64_blocked, 64),
            "blocked64_128": wrap(oracle.matrix_inv_64_blocked, 128)}


def test_canon_is_canonical_bytes_for_fp32():
    x = np.array([0.0, -0.0, 1.5, -2.0 ** -140, np.inf], np.float32)
    assert canon(x) == canonical_bytes(x) == np.array([0.0, 0.0, 1.5, -2.0 ** -140, np.inf], np.float32).tobytes()
    y = np.array([-0.0, 2.0 ** -900], np.float64)
    assert canon(y) == np.array([0.0, 2.0 ** -900], np.float64).tobytes()


def _singular_inputs(n, dtype):
    out = {}
    for k in sorted({0, n // 2, n - 1}):
        out[f"zero_column[{k}]"] = zero_column(n, k, 100 + n, dtype)
        out[f"zero_row[{k}]"] = zero_row(n, k, 200 + n, dtype)
    for k in sorted({0, (n - 2) // 2, n - 2}):
        if n >= 2:
            out[f"ones_block[{k}]"] = ones_block(n, k, 300 + n, dtype)
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("n", ORDERS)
def test_singular_by_construction_is_status_2_in_every_form(oracle, n, dtype):
    for name, a in _singular_inputs(n, dtype).items():
        assert a.dtype == dtype and np.isfinite(a).all()
        for form, fn in oracle_forms(oracle, dtype).items():
            assert fn(a, n)[1] == STATUS_SINGULAR == oracle.STATUS_SINGULAR, (name, n, form)


def test_singular_families_fail_late(oracle):
    """The point of these inputs: the first bad pivot is met at the stated step, not at step 0 or 1.  Up to there the
    elimination is that of the matrix with the zero column (row) replaced by a unit column (row), which is regular."""
    n = 40
    for k in (7, 39):
        a = zero_column(n, k, 5)
        assert (a[:, k] == 0).all() and np.linalg.matrix_rank(a.astype(np.float64)) == n - 1
        assert np.linalg.matrix_rank(np.delete(a, k, axis=1).astype(np.float64)[:, :k]) == k   # k good pivots first
    a = zero_row(n, 0, 5)
    assert np.linalg.matrix_rank(a.astype(np.float64)) == n - 1
    a = ones_block(n, 20, 5)
    assert np.linalg.matrix_rank(a.astype(np.float64)) == n - 1 and (a[20:22, 20:22] == 1).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("n", ORDERS)
def test_exact_families_have_the_written_down_inverse_in_every_form(oracle, n, dtype):
    for name, (a, x) in exact_families(n, 400 + n, dtype).items():
        assert a.dtype == dtype and x.dtype == dtype and a.shape == x.shape == (n, n)
        # the written-down inverse is an inverse: the products are exact in float64 for every family
        assert np.array_equal(a.astype(np.float64) @ x.astype(np.float64), np.eye(n)), (name, n)
        for form, fn in oracle_forms(oracle, dtype).items():
            got, st = fn(a, n)
            assert st == STATUS_OK, (name, n, form)
            assert canon(got) == canon(x), (name, n, form)


def test_negative_zero_variant_really_holds_negative_zeros():
    a, _ = exact_families(17, 1)["perm-0"]
    assert np.signbit(a[a == 0]).all() and (a == 0).sum() == 17 * 16
    a, _ = exact_families(17, 1)["perm"]
    assert not np.signbit(a[a == 0]).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("orders", [[1, 2, 3], [5, 64, 1, 17], [65, 8, 128, 40, 16], [100, 100, 57]],
                         ids=lambda o: "-".join(map(str, o)))
def test_block_diagonal_inverse_is_the_blocks_inverses(oracle, orders, dtype):
    a, blocks = block_diagonal(orders, 500, dtype)
    n = sum(orders)
    forms = oracle_forms(oracle, dtype)
    step = forms["inplace" if dtype == np.float32 else "inplace64"]
    inv_blocks = []
    for b in blocks:
        x, st = step(b, b.shape[0])
        assert st == STATUS_OK
        inv_blocks.append(x.reshape(b.shape))
    want = place_blocks(inv_blocks)
    # the step-by-step forms (and their bit-identical cache-blocked evaluation) reproduce it bit for bit; the fp64
    # rank-bw mirror sums in another order and is held to that order by its own tests
    for form, fn in forms.items():
        if form.startswith("blocked64"):
            continue
        got, st = fn(a, n)
        assert st == STATUS_OK and canon(got) == canon(want), (orders, form)


@pytest.mark.parametrize("n", [3, 8, 40, 100, 300])
def test_duplicate_rows_is_status_0_and_finite_in_fp32(oracle, n):
    a = duplicate_rows(n, 600 + n)
    assert np.array_equal(a[0], a[n - 1])
    forms = oracle_forms(oracle, np.float32)
    want, st = forms["inplace"](a, n)
    assert st == STATUS_OK and np.isfinite(want).all()
    for form, fn in forms.items():
        got, st = fn(a, n)
        assert st == STATUS_OK and canon(got) == canon(want), (n, form)


def test_overflow_list_holds_both_outcomes_and_never_ok_with_a_nonfinite_inverse(oracle):
    seen = collections.Counter()
    assert len(set(OVERFLOW_LIST)) == len(OVERFLOW_LIST)
    for n, seed, mode, k, want in OVERFLOW_LIST:
        a = overflow(n, seed, mode, k)
        assert a.dtype == np.float32 and np.isfinite(a).all()
        ref = None
        for form, fn in oracle_forms(oracle, np.float32).items():
            x, st = fn(a, n)
            assert st == want, (n, seed, mode, k, form)
            if st == STATUS_OK:
                assert np.isfinite(x).all(), (n, seed, mode, k, form)      # never "OK with inf"
                ref = x if ref is None else ref
                assert canon(x) == canon(ref), (n, seed, mode, k, form)
        seen[(n, want)] += 1
    for n in (8, 40, 100, 200):
        assert seen[(n, STATUS_OK)] >= 1 and seen[(n, STATUS_SINGULAR)] >= 1, (n, seen)
    assert sum(v for (n, s), v in seen.items() if s == STATUS_OK) >= 5
    assert sum(v for (n, s), v in seen.items() if s == STATUS_SINGULAR) >= 5


def test_gate_blocks_are_regular(oracle):
    """The valid members the GPU batches put beside the singular ones."""
    for n in (3, 8, 64, 65, 128, 300):
        assert oracle.matrix_inv_32_inplace(gate_matrix(n, 900 + n), n, return_info=True)[1]["status"] == STATUS_OK
