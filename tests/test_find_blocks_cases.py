"""CPU checks of tests/find_blocks_cases.py itself: the NumPy mirror of the block finder against a brute-force
restatement that shares nothing with it -- rows compared as Python tuples, supervariables packed by an explicit greedy
loop -- and the invariants of every case the GPU tests use.  Array equality throughout."""
import numpy as np
import pytest

import find_blocks_cases as F

CHUNK = 3968           # the GPU tests read the library's; the builders only need something large enough here


def brute_orders(case, max_order, agglomerate):
    rows = [tuple(case.col[case.crow[i]:case.crow[i + 1]].tolist()) for i in range(case.n)]
    sizes = []                                          # supervariables: equal consecutive rows, at most max_order
    for i, row in enumerate(rows):
        if i > 0 and row == rows[i - 1] and sizes[-1] < max_order:
            sizes[-1] += 1
        else:
            sizes.append(1)
    if not agglomerate:
        return np.array(sizes, np.int32)
    blocks = [0]                                        # greedy: a block takes supervariables while they fit
    for s in sizes:
        if blocks[-1] and blocks[-1] + s > max_order:
            blocks.append(0)
        blocks[-1] += s
    return np.array(blocks, np.int32)


def small_cases():
    rng = np.random.default_rng(7400)
    yield "one row", F.common_pattern_case(1)
    yield "two equal rows", F.common_pattern_case(2)
    yield "two different rows", F.tridiagonal_case(2)
    yield "common 131", F.common_pattern_case(131)
    yield "tridiagonal 131", F.tridiagonal_case(131)
    yield "one entry", F.one_entry_case()
    yield "stencil 3", F.stencil27_case((4, 3, 3), 3)
    yield "stencil 5", F.stencil27_case((3, 3, 2), 5)
    yield "runs", F.runs_case(rng.integers(1, 12, 60), 7401)
    yield "long runs", F.runs_case(rng.integers(1, 300, 12), 7402)


@pytest.mark.parametrize("max_order", F.MAX_ORDERS)
def test_mirror_is_the_brute_force_restatement(max_order):
    for name, case in small_cases():
        for agglomerate in (False, True):
            got = F.orders_of(F.mirror_starts(case.crow, case.col, max_order, agglomerate, case.nat))
            assert np.array_equal(got, brute_orders(case, max_order, agglomerate)), (name, max_order, agglomerate)


@pytest.mark.parametrize("max_order", F.MAX_ORDERS)
def test_invariants_of_every_case(max_order):
    cases = [case for _, case in small_cases()]
    cases += [F.seams_case(CHUNK, max_order, kind) for kind in F.SEAM_KINDS]
    for case in cases:
        F.check_invariants(case, max_order)


def test_long_chain_case_invariants():
    case = F.long_chain_case(CHUNK)
    assert case.n >= 64 * CHUNK and 4.5 < case.col.size / case.n < 5.5
    F.check_invariants(case, 32)


def test_named_properties():
    # a run of n rows is cut every max_order rows; merging cannot put two full supervariables together
    case = F.common_pattern_case(131)
    for agglomerate in (False, True):
        assert F.orders_of(F.mirror_starts(case.crow, case.col, 32, agglomerate)).tolist() == [32, 32, 32, 32, 3]
    # single rows are merged into full blocks, the last one takes what is left
    case = F.tridiagonal_case(131)
    assert F.orders_of(F.mirror_starts(case.crow, case.col, 32, False)).tolist() == [1] * 131
    assert F.orders_of(F.mirror_starts(case.crow, case.col, 32, True)).tolist() == [32, 32, 32, 32, 3]
    # node blocks: the unknowns of a node, then ten (six) nodes to a block of 30
    for dof, grid in ((3, (4, 5, 2)), (5, (3, 2, 2))):
        case = F.stencil27_case(grid, dof)
        assert set(F.orders_of(F.mirror_starts(case.crow, case.col, 32, False)).tolist()) == {dof}
        assert set(F.orders_of(F.mirror_starts(case.crow, case.col, 32, True)).tolist()) == {30}
    # the same set in another stored order is a boundary
    case = F.one_entry_case()
    assert case.nat[20] == 1 and case.nat[22] == 0
