"""Launch planning of the dense calls, host only (a null handle: default settings, no device).

Every answer of the mi32_resolve_* queries and of mi32_workspace_bytes, over the orders at which a path or a padding
changes and every value of the knobs MI32_ALGO, MI32_BLOCK_W64 and MI32_BLOCK_W, equals the table
tests/golden/dense_route_table.json.  The table was recorded by tools/dense_route_table.py from a build of the commit
it names -- the parent of the change that introduced the DenseRoute -- never from the code under test; it is stored
without its repetitions (pack / unpack there).  The second half
reads the DenseRoute itself (mi32_debug_dense_route, tests only): what a det call is told about the pivot list of each
path, and that a path plans nothing it does not run."""
import ctypes
import importlib.util
import json
import os

import pytest

from gpu_matrix_inversion_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("dense_route_table", os.path.join(ROOT, "tools", "dense_route_table.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(ROOT, "tests", "golden", "dense_route_table.json")) as f:
    PACKED = json.load(f)
TABLE = gen.unpack(PACKED)  # {"algo/w64/w": {"n/batch": [an answer per gen.COLUMNS entry]}}

RESIDENT, WORKGROUP, SWEEP, BLOCKED32, BLOCKED64, NOPIVOT64 = range(6)  # DenseRoute::Path


@pytest.fixture
def clean_env(monkeypatch):
    """No planning knob set but the ones a test sets through gen.set_knobs; monkeypatch puts every variable it was
    told about back afterwards, whatever os.environ went through in between."""
    for name in {k for k in os.environ if k.startswith("MI32_")} | {name for name, _ in gen.KNOBS}:
        monkeypatch.delenv(name, raising=False)


def test_table_names_its_commit_and_covers_every_case():
    assert len(PACKED["commit"]) == 40 and int(PACKED["commit"], 16) >= 0
    assert gen.ORDERS == (1, 31, 32, 33, 64, 65, 128, 129, 255, 256, 257, 511, 512, 513, 1000, 4096, 4097, 4200, 8200,
                          16384, 16385)
    assert gen.BATCHES == (1, 4, 8, 64)
    assert dict(gen.KNOBS) == {"MI32_ALGO": (None, 1, 2, 3, 4), "MI32_BLOCK_W64": (None, 64, 128, 256),
                               "MI32_BLOCK_W": (None, 128)}
    assert len(TABLE) == 5 * 4 * 2
    assert all(len(rows) == len(gen.ORDERS) * len(gen.BATCHES) for rows in TABLE.values())
    assert all(len(row) == len(gen.COLUMNS) for rows in TABLE.values() for row in rows.values())
    assert gen.pack(TABLE) == {name: PACKED[name] for name in gen.COLUMNS}


def test_planning_answers_equal_the_recorded_table(clean_env):
    got = gen.table(gen.bind(_lib.LIB_PATH))
    assert got.keys() == TABLE.keys()
    for knobs, rows in TABLE.items():
        for shape, want in rows.items():
            assert got[knobs][shape] == want, f"MI32_ALGO/MI32_BLOCK_W64/MI32_BLOCK_W = {knobs}, n/batch = {shape}"


def dense_route(lib, n, batch, elem_bytes, handle=None):
    out, ws = (ctypes.c_int * 5)(), ctypes.c_size_t()
    fn = lib.mi32_debug_dense_route
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                   ctypes.POINTER(ctypes.c_size_t)]
    assert fn(handle, n, batch, elem_bytes, out, ctypes.byref(ws)) == 0
    return dict(path=out[0], det_steps=out[1], det_first=out[2], np=out[3], bw=out[4], ws=ws.value)


@pytest.mark.parametrize("algo", gen.KNOBS[0][1])
def test_dense_route_of_every_shape(clean_env, algo):
    """Per path: the pivot list of a det call and its first real step, the plan the path carries, and the agreement of
    the DenseRoute with the public queries (which the table above pins).  (The no-pivot paths are a context's setting,
    not a knob: a null handle does not reach them.)"""
    lib = _lib.load()
    gen.set_knobs((algo, None, None))
    for n in gen.ORDERS:
        for batch in gen.BATCHES:
            for elem_bytes in (4, 8):
                d = dense_route(lib, n, batch, elem_bytes)
                where = f"n {n} batch {batch} elem_bytes {elem_bytes} MI32_ALGO {algo}"
                if elem_bytes == 4:
                    resolved = lib.mi32_resolve_algo(None, n, batch)
                    assert d["path"] == {_lib.ALGO_RESIDENT: RESIDENT, _lib.ALGO_WORKGROUP: WORKGROUP,
                                         _lib.ALGO_SWEEP: SWEEP, _lib.ALGO_BLOCKED: BLOCKED32}[resolved], where
                    assert d["ws"] == lib.mi32_workspace_bytes(n, batch, 0), where
                else:
                    assert d["path"] in (RESIDENT, WORKGROUP, SWEEP, BLOCKED64), where
                    bw64 = ctypes.c_int()
                    assert lib.mi32_resolve_blocking_f64(None, n, ctypes.byref(bw64)) == 0
                    assert bw64.value == (d["bw"] if d["path"] == BLOCKED64 else 0), where
                    if d["path"] in (RESIDENT, WORKGROUP):
                        assert d["ws"] == 0, where  # the fp64 one-launch calls ensure no workspace
                if d["path"] in (RESIDENT, WORKGROUP):
                    assert n <= (64 if d["path"] == RESIDENT else 128), where
                    assert (d["det_steps"], d["det_first"], d["np"], d["bw"]) == (0, 0, 0, 0), where
                elif d["path"] == SWEEP:  # no padding, no blocked route
                    assert (d["det_steps"], d["det_first"], d["np"], d["bw"]) == (n, 0, 0, 0), where
                elif d["path"] == BLOCKED32:  # the padding comes first
                    route, _ = _lib.resolve_route(None, n, batch)
                    assert (d["np"], d["bw"]) == (route["np"], route["block_width"]), where
                    assert (d["det_steps"], d["det_first"]) == (d["np"], d["np"] - n), where
                else:  # the fp64 blocked paths pad behind the matrix
                    assert d["np"] >= n and d["np"] % d["bw"] == 0, where
                    assert (d["det_steps"], d["det_first"]) == (d["np"], 0), where
