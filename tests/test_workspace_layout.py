"""The workspace layout, host only (a null handle: default settings, no device): what ``mi32_debug_ws_layout`` lists for
every shape of tools/dense_route_table.py's ORDERS x BATCHES, both element sizes and the knob values of that table.

Guard off: the regions of every carve are contiguous from offset 0 on 256-byte boundaries and end where the
``DenseRoute``'s workspace ends; the golden route table is another test's (tests/test_dense_route.py) and is not touched.
Guard on (64 KiB): the same names, order, sizes and kinds, every gap exactly one zone, and the size queries report the
guarded total -- while planning answers what it answered without the guard.
"""
import ctypes
import importlib.util
import os

import pytest

import workspace_cases as W
from gpu_matrix_inversion_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("dense_route_table", os.path.join(ROOT, "tools", "dense_route_table.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

KNOB_SETS = [(a, w64, w) for a in gen.KNOBS[0][1] for w64 in gen.KNOBS[1][1] for w in gen.KNOBS[2][1]]
SHAPES = [(n, b, es) for n in gen.ORDERS for b in gen.BATCHES for es in (4, 8)]


@pytest.fixture
def lib(monkeypatch):
    """The library with the tests-only entry points bound, no planning knob set, and the guard off again afterwards
    whatever the test did."""
    for name in {k for k in os.environ if k.startswith("MI32_")} | {name for name, _ in gen.KNOBS}:
        monkeypatch.delenv(name, raising=False)
    lib = W.bind(_lib.load())
    try:
        yield lib
    finally:
        assert lib.mi32_debug_ws_guard(0) == 0
        gen.set_knobs((None, None, None))


def knob_id(k):
    return "/".join("-" if v is None else str(v) for v in k)


def expected_names(route, owner):
    return {W.INVERSE: W.REGIONS.get(route["path"], ()), W.DET: W.DET_REGIONS, W.RESIDUAL: W.RESIDUAL_REGIONS}[owner]


@pytest.mark.parametrize("knobs", KNOB_SETS, ids=knob_id)
def test_layout_without_and_with_the_guard(lib, knobs):
    gen.set_knobs(knobs)
    G = W.G_HOST
    for n, batch, es in SHAPES:
        where = f"n {n} batch {batch} elem_bytes {es} knobs {knob_id(knobs)}"
        route = W.dense_route(lib, None, n, batch, es)
        plain = W.layout(lib, None, n, batch, es)
        groups = W.carves(plain)
        owners = [key[0] for key, _ in groups]
        # ---- which carves there are
        parts = []
        if route["path"] in W.ONE_LAUNCH:  # nothing beyond the residual share
            assert owners == ([W.RESIDUAL] if es == 4 else []), where
            assert route["ws"] == (plain[-1].offset + plain[-1].bytes if es == 4 else 0), where
        else:
            parts = [key for key, _ in groups if key[0] == W.INVERSE]
            assert parts in ([(W.INVERSE, 0)], [(W.INVERSE, 0), (W.INVERSE, 1)]), where
            assert owners == [W.INVERSE] * len(parts) + [W.DET] + ([W.RESIDUAL] if es == 4 else []), where
            if route["path"] == W.BLOCKED32:
                assert len(parts) == _lib.resolve_route(None, n, batch)[0]["parts"], where
            else:
                assert len(parts) == 1, where
        # ---- guard off: contiguous from the carve's start, 256-byte offsets, names and kinds as documented
        ends = {}
        for (owner, part), regs in groups:
            assert tuple(r.name for r in regs) == expected_names(route, owner), where
            at = ends.get((W.INVERSE, 0), 0) if (owner, part) == (W.INVERSE, 1) else 0
            for r in regs:
                assert r.offset == at and r.offset % 256 == 0 and r.bytes > 0 and r.bytes % 256 == 0, (where, r)
                assert r.kind == W.KIND_OF[r.name], (where, r)
                # a whole number of elements (the residual's sums and the fp64 routes' values are doubles)
                if r.kind == W.VALUES:
                    assert r.bytes % (8 if owner == W.RESIDUAL else es) == 0, (where, r)
                members = batch if owner != W.INVERSE or len(parts) == 1 else (batch + 1) // 2 if part == 0 else batch // 2
                if r.name in W.PER_MEMBER or r.name == "piv" and owner == W.DET:
                    assert r.bytes % members == 0 and (r.bytes // members) % 256 == 0, (where, r, members)
                at += r.bytes
            ends[(owner, part)] = at
        if route["path"] not in W.ONE_LAUNCH:
            # the last region ends where the workspace ends; the two parts of a split batch add up to it
            last = ends[(W.INVERSE, 1)] if (W.INVERSE, 1) in ends else ends[(W.INVERSE, 0)]
            assert last == route["ws"], (where, last, route["ws"])
            if es == 4:
                assert route["ws"] == lib.mi32_workspace_bytes(n, batch, 0), where
                assert ends[(W.RESIDUAL, 0)] <= route["ws"], where
        # ---- guard on: the same regions, one zone in front of each carve and one behind every region
        algo = lib.mi32_resolve_algo(None, n, batch)
        bw64 = ctypes.c_int()
        assert lib.mi32_resolve_blocking_f64(None, n, ctypes.byref(bw64)) == 0
        blocked = _lib.resolve_route(None, n, batch) if n <= 16384 else None
        with W.guard(lib, G) as g:
            assert g == G
            guarded = W.layout(lib, None, n, batch, es)
            groute = W.dense_route(lib, None, n, batch, es)
            gws = lib.mi32_workspace_bytes(n, batch, 0)
            assert lib.mi32_resolve_algo(None, n, batch) == algo, where
            g64 = ctypes.c_int()
            assert lib.mi32_resolve_blocking_f64(None, n, ctypes.byref(g64)) == 0 and g64.value == bw64.value, where
            assert (_lib.resolve_route(None, n, batch) if n <= 16384 else None) == blocked, where
        assert {k: v for k, v in groute.items() if k != "ws"} == {k: v for k, v in route.items() if k != "ws"}, where
        assert [(e.owner, e.part, e.name, e.bytes, e.kind) for e in guarded] == \
               [(e.owner, e.part, e.name, e.bytes, e.kind) for e in plain], where
        gends = {}
        for (owner, part), regs in W.carves(guarded):
            start = gends.get((W.INVERSE, 0), 0) if (owner, part) == (W.INVERSE, 1) else 0
            at = start + G
            for r in regs:
                assert r.offset == at, (where, r, at)   # every gap is exactly G
                at += r.bytes + G
            gends[(owner, part)] = at
            assert at - start == ends[(owner, part)] - (ends[(W.INVERSE, 0)] if (owner, part) == (W.INVERSE, 1) else 0) \
                + (len(regs) + 1) * G, where
        if route["path"] in W.ONE_LAUNCH:
            assert groute["ws"] == (gends[(W.RESIDUAL, 0)] if es == 4 else 0), where
        else:
            n_carves = 2 if (W.INVERSE, 1) in gends else 1
            n_regions = len(expected_names(route, W.INVERSE))
            assert groute["ws"] == route["ws"] + n_carves * (n_regions + 1) * G, (where, groute["ws"], route["ws"])
            assert groute["ws"] == gends[(W.INVERSE, n_carves - 1)], where
        if es == 4:
            assert gws == groute["ws"], where
    assert lib.mi32_workspace_bytes(256, 1, 0) == W.dense_route(lib, None, 256, 1, 4)["ws"]  # the guard is off again


def test_the_guard_size_is_rounded_up_to_256(lib):
    plain = lib.mi32_workspace_bytes(300, 1, 0)
    regions = len(W.BLOCKED32_REGIONS)
    for asked, got in ((1, 256), (256, 256), (257, 512), (65536, 65536)):
        with W.guard(lib, asked) as g:
            assert g == got
            assert lib.mi32_workspace_bytes(300, 1, 0) == plain + (regions + 1) * got
            assert W.layout(lib, None, 300, 1, 4)[0].offset == got
        assert lib.mi32_workspace_bytes(300, 1, 0) == plain


def test_layout_refuses_bad_arguments(lib):
    count = ctypes.c_int(-1)
    regions = (W.Region * 4)()
    fn = lib.mi32_debug_ws_layout
    assert fn(None, 0, 1, 4, regions, 4, ctypes.byref(count)) != 0
    assert fn(None, 8, 0, 4, regions, 4, ctypes.byref(count)) != 0
    assert fn(None, 8, 1, 2, regions, 4, ctypes.byref(count)) != 0
    assert fn(None, 8, 1, 4, regions, 4, None) != 0
    assert fn(None, 8, 1, 4, None, 4, ctypes.byref(count)) != 0
    assert count.value == -1
    # a short array takes what fits; the count is the number there are
    assert fn(None, 300, 1, 4, regions, 4, ctypes.byref(count)) == 0
    assert count.value == len(W.BLOCKED32_REGIONS) + len(W.DET_REGIONS) + len(W.RESIDUAL_REGIONS)
    assert [r.name.decode() for r in regions] == list(W.BLOCKED32_REGIONS[:4])
    report = W.Report()
    assert lib.mi32_debug_ws_check(None, ctypes.byref(report)) != 0 and lib.mi32_debug_ws_poke(None, 0, 0, 1) != 0
