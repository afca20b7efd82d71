"""Inputs and helpers of the variable-size solve tests (tests/test_vsolve_abi.py, tests/test_gpu_vsolve.py): the dispatch
rule of mi32_solve_device_vbatched restated from the uniform call's rule (solve_cases.cap / lanes_of / rows_of), and the
packed right-hand side of ``Inverter.solve_ragged``."""
import numpy as np

from solve_cases import cap, lanes_of, mirror_solve, rhs, rows_of


def chunks_of(n, nrhs):
    """The launches mi32_solve_device makes for a uniform batch of order n: [(col0, cols, lanes, rows)], full chunks
    first; lanes is 0 for the workgroup-resident kernel, rows 0 for the register-resident one."""
    out = []
    for col0 in range(0, nrhs, cap(n)):
        cols = min(cap(n), nrhs - col0)
        resident = n + cols <= 64
        out.append((col0, cols, lanes_of(n + cols) if resident else 0, 0 if resident else rows_of(n)))
    return out


def expected_launches(orders, nrhs):
    """[(first, count, col0, cols, lanes, rows)] of mi32_vbatch_solve_launches: one launch per chunk of every maximal
    run of consecutive members of the list sorted by order whose chunk sequences agree, by first, then by col0."""
    srt = sorted(int(n) for n in orders)
    out, first = [], 0
    while first < len(srt):
        seq = chunks_of(srt[first], nrhs)
        end = first + 1
        while end < len(srt) and (srt[end] == srt[end - 1] or chunks_of(srt[end], nrhs) == seq):
            end += 1
        out += [(first, end - first) + c for c in seq]
        first = end
    return out


def row_offsets(orders):
    """Where each member's rows start in the packed right-hand side, and the total."""
    o = np.asarray(orders, np.int64)
    return np.concatenate(([0], np.cumsum(o)))


def packed_rhs(orders, k, seed, dtype=np.float32):
    """The (sum of the orders, k) right-hand side of solve_ragged: member i's rows are rhs(n_i, k, seed + i)."""
    return np.concatenate([rhs(int(n), k, seed + i, dtype) for i, n in enumerate(orders)])


def mirror_members(dll, mats, b, pivoting=True):
    """(packed X, statuses) of the mirror, member by member, for the packed right-hand side b (rows, k)."""
    off = row_offsets([m.shape[0] for m in mats])
    x = np.empty_like(b)
    st = np.empty(len(mats), np.int32)
    for i, m in enumerate(mats):
        x[off[i]:off[i + 1]], st[i] = mirror_solve(dll, m, b[off[i]:off[i + 1]], pivoting)
    return x, st
