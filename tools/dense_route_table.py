"""Record what launch planning answers for every dense shape and knob of tests/test_dense_route.py.

    python tools/dense_route_table.py LIB.so COMMIT > tests/golden/dense_route_table.json

LIB.so is a build of the commit the table pins (the parent of the change under test, never the tree under test);
COMMIT is its hash, kept in the file.  Host only: a null handle, so default settings, and no device.  The planning
functions read the environment on every call, so one process walks all the knob values.
"""
import ctypes
import json
import os
import sys

ORDERS = (1, 31, 32, 33, 64, 65, 128, 129, 255, 256, 257, 511, 512, 513, 1000, 4096, 4097, 4200, 8200, 16384, 16385)
BATCHES = (1, 4, 8, 64)
KNOBS = (("MI32_ALGO", (None, 1, 2, 3, 4)), ("MI32_BLOCK_W64", (None, 64, 128, 256)), ("MI32_BLOCK_W", (None, 128)))
COLUMNS = ("resolve_algo", "workspace_bytes", "block_width_f64", "panel_width", "block_width", "route")
ROUTE_FIELDS = ("np", "block_width", "nblocks", "shared_panels", "lookahead", "parts", "part_batch",
                "part_strips_at_end", "first_fused_block")


class Route(ctypes.Structure):  # mi32_route_t
    _fields_ = [("np", ctypes.c_int), ("block_width", ctypes.c_int), ("nblocks", ctypes.c_int),
                ("shared_panels", ctypes.c_int), ("lookahead", ctypes.c_int), ("parts", ctypes.c_int),
                ("part_batch", ctypes.c_int * 2), ("part_strips_at_end", ctypes.c_int * 2),
                ("first_fused_block", ctypes.c_int)]


def bind(path):
    lib = ctypes.CDLL(path)
    ip, vp = ctypes.POINTER(ctypes.c_int), ctypes.c_void_p
    lib.mi32_workspace_bytes.restype = ctypes.c_size_t
    lib.mi32_workspace_bytes.argtypes = [ctypes.c_int] * 3
    lib.mi32_resolve_algo.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    lib.mi32_resolve_blocking.argtypes = [vp, ctypes.c_int, ctypes.c_int, ip, ip]
    lib.mi32_resolve_blocking_f64.argtypes = [vp, ctypes.c_int, ip]
    lib.mi32_resolve_route.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(Route), ip, ctypes.c_int]
    return lib


def set_knobs(values):
    for (name, _), v in zip(KNOBS, values):
        if v is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = str(v)


def answers(lib, n, batch, algo):
    """One row, a value per COLUMNS entry; the route as the mi32_route_t fields in order, then the workgroups per panel
    of every outer block (None where the blocked fp32 path does not take the order)."""
    w, bw, bw64 = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.mi32_resolve_blocking_f64(None, n, ctypes.byref(bw64)) == 0
    assert lib.mi32_resolve_blocking(None, n, batch, ctypes.byref(w), ctypes.byref(bw)) == 0
    r, groups = Route(), (ctypes.c_int * 128)()
    route = None
    if lib.mi32_resolve_route(None, n, batch, ctypes.byref(r), groups, 128) == 0:  # blocked_supported(n)
        route = [list(v) if hasattr(v, "__len__") else v for v in (getattr(r, f) for f in ROUTE_FIELDS)]
        route.append([groups[b] for b in range(r.nblocks)])
    return [lib.mi32_resolve_algo(None, n, batch), lib.mi32_workspace_bytes(n, batch, algo or 0), bw64.value, w.value,
            bw.value, route]


def table(lib):
    """{"algo/w64/w": {"n/batch": row}} over every knob value ("-": unset), order and batch size."""
    out = {}
    for algo in KNOBS[0][1]:
        for w64 in KNOBS[1][1]:
            for w in KNOBS[2][1]:
                set_knobs((algo, w64, w))
                key = "/".join("-" if v is None else str(v) for v in (algo, w64, w))
                out[key] = {f"{n}/{b}": answers(lib, n, b, algo) for n in ORDERS for b in BATCHES}
    set_knobs((None, None, None))
    return out


def pack(full):
    """The table without its repetitions, losslessly: per column the distinct answers ("values"), the distinct lists of
    indices into them over the shapes in table()'s order ("shapes"), and which list each knob setting has ("knobs",
    in table()'s order) -- most answers do not move with most knobs."""
    doc = {}
    for c, name in enumerate(COLUMNS):
        values, lists, knobs = [], [], []
        for rows in full.values():
            idx = []
            for row in rows.values():
                if row[c] not in values:
                    values.append(row[c])
                idx.append(values.index(row[c]))
            if idx not in lists:
                lists.append(idx)
            knobs.append(lists.index(idx))
        doc[name] = {"values": values, "shapes": lists, "knobs": knobs}
    return doc


def unpack(doc):
    """pack's inverse, keyed as table() keys its result."""
    knob_keys = ["/".join("-" if v is None else str(v) for v in (a, b, c))
                 for a in KNOBS[0][1] for b in KNOBS[1][1] for c in KNOBS[2][1]]
    shape_keys = [f"{n}/{b}" for n in ORDERS for b in BATCHES]
    cols = [doc[name] for name in COLUMNS]
    return {k: {s: [col["values"][col["shapes"][col["knobs"][i]][j]] for col in cols] for j, s in enumerate(shape_keys)}
            for i, k in enumerate(knob_keys)}


def dump(doc, out):
    """One value or index list per line: a change to the table shows as the lines that moved."""
    lines = lambda items: ",\n  ".join(json.dumps(v, separators=(",", ":")) for v in items)  # noqa: E731
    out.write('{"commit": %s' % json.dumps(doc["commit"]))
    for name in COLUMNS:
        col = doc[name]
        out.write(',\n"%s": {\n "values": [\n  %s],\n "shapes": [\n  %s],\n "knobs": %s}'
                  % (name, lines(col["values"]), lines(col["shapes"]), json.dumps(col["knobs"], separators=(",", ":"))))
    out.write("}\n")


if __name__ == "__main__":
    full = table(bind(sys.argv[1]))
    assert unpack(pack(full)) == full
    dump(dict(pack(full), commit=sys.argv[2]), sys.stdout)
