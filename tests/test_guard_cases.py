"""Host-only proof of the checker in tests/guard_cases.py: what ``carve`` lays out, and that ``intact`` finds and locates
a single changed margin element wherever it is.  The kernels are not involved."""
import numpy as np
import pytest

import guard_cases as G
import overflow_cases as ovf
import residual_cases
import wide_cases

DTYPES = [G.F32, G.F64, G.I32]
IDS = ["fp32", "fp64", "int32"]


def fill_of(dtype, kind="out"):
    return G.NAN_IN[dtype] if kind == "in" else G.SENTINEL[dtype]


def carved(dtype, lead=G.LEAD_ODD, shape=(3, 5, 5), margin=None):
    margin = G.margin_for(shape[-1]) if margin is None else margin
    whole, view = G.carve(shape, dtype, lead, fill_of(dtype), margin)
    return whole, view, G.span(whole, view)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("lead", [0, G.LEAD_ODD, 3, G.LEAD_ALIGNED])
def test_layout(dtype, lead):
    shape, margin = (3, 5, 5), G.margin_for(5)
    whole, view, (off, size) = carved(dtype, lead)
    assert whole.ndim == 1 and whole.dtype == dtype and view.shape == shape and view.dtype == dtype
    assert size == 75 and off == G.front(margin) + lead and G.front(margin) % G.ALIGN == 0
    assert off >= margin and whole.size - off - size >= margin            # a full margin on either side
    assert np.shares_memory(whole, view) and view.flags.c_contiguous
    assert (G.bits_of(whole) == fill_of(dtype)).all()                     # the view's own elements included
    view[...] = 1                                                         # writing the view leaves the margins alone
    assert G.intact(whole, (off, size), fill_of(dtype)) == (True, None, 0)
    assert (whole[off:off + size] == 1).all()


def test_the_plain_reading_without_a_margin():
    whole, view = G.carve((4,), G.F32, 1, G.SENTINEL[G.F32])
    assert G.span(whole, view) == (1, 4) and whole.size == 6


@pytest.mark.parametrize("dtype", [G.F32, G.F64], ids=["fp32", "fp64"])
def test_lead_one_is_element_aligned_and_nothing_more(dtype):
    """With the whole buffer at an allocation's start (256 bytes or better), the odd view's address is one element
    mod 16 bytes and the control's is a multiple of 256."""
    es = np.dtype(dtype).itemsize
    for margin in (0, 1, 63, 64, 65, G.margin_for(300), G.margin_for(127, 3)):
        whole, view = G.carve((2, 3), dtype, G.LEAD_ODD, fill_of(dtype), margin)
        assert (G.span(whole, view)[0] * es) % 16 == es
        whole, view = G.carve((2, 3), dtype, G.LEAD_ALIGNED, fill_of(dtype), margin)
        assert (G.span(whole, view)[0] * es) % 256 == 0


def test_margin_is_two_members_and_two_padded_rows():
    for n, cols, padded in ((1, None, 512), (64, None, 512), (300, None, 512), (520, None, 1024), (640, None, 1024),
                            (127, 3, 512), (8, 600, 1024)):
        c = n if cols is None else cols
        assert G.margin_for(n, cols) == 2 * n * c + 2 * padded and padded >= max(n, c) and padded % 512 == 0
    # no route pads further than the next multiple of 512: the one-launch classes, the wide path's 160 ... 256, the fp64
    # blocks of 64 / 128 / 256 columns and the fp32 outer blocks of at most 512
    assert all(p <= 512 for p in (8, 16, 32, 64, 80, 96, 112, 128, 160, 192, 224, 256))


def positions(off, size, total):
    """The first, last and middle element of either margin (the last of the front one is the element just in front of
    the view, the first of the back one the element just behind it)."""
    back = off + size
    return {"front first": 0, "front middle": off // 2, "just in front": off - 1, "just behind": back,
            "back middle": (back + total) // 2, "back last": total - 1}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("lead", [G.LEAD_ODD, G.LEAD_ALIGNED])
def test_one_flipped_element_is_found_and_located(dtype, lead):
    whole, view, (off, size) = carved(dtype, lead)
    where = positions(off, size, whole.size)
    assert where["just in front"] - off == -1 and where["just behind"] - off == size
    assert len(set(where.values())) == 6
    for name, i in where.items():
        w = whole.copy()
        G.bits_of(w)[i] ^= 1                                              # the lowest bit only
        r = G.intact(w, (off, size), fill_of(dtype))
        assert r == (False, i - off, 1), (name, r)
        assert (r.first < 0) == (i < off) and (r.first >= size) == (i >= off + size)
    assert G.intact(whole, (off, size), fill_of(dtype)).ok


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_several_changes_are_counted_from_the_first(dtype):
    whole, view, (off, size) = carved(dtype)
    w = whole.copy()
    for i in (off - 7, off - 2, off + size + 4):
        G.bits_of(w)[i] = 0
    G.bits_of(w)[off + 1] = 0                                             # inside the view: not a margin
    assert G.intact(w, (off, size), fill_of(dtype)) == (False, -7, 3)


@pytest.mark.parametrize("dtype", [G.F32, G.F64], ids=["fp32", "fp64"])
def test_a_nan_whose_payload_changed_is_found(dtype):
    fill = G.NAN_IN[dtype]
    whole, view = G.carve((4, 4), dtype, G.LEAD_ODD, fill, 40)
    off, size = G.span(whole, view)
    assert np.isnan(whole).all()
    w = whole.copy()
    G.bits_of(w)[off - 3] = fill ^ 0x10                                   # still a quiet NaN, another payload
    assert np.isnan(w).all() and G.intact(w, (off, size), fill) == (False, -3, 1)
    w = whole.copy()
    w[off + size + 2] = np.nan                                            # the default NaN: no payload
    assert G.intact(w, (off, size), fill) == (False, size + 2, 1)


@pytest.mark.parametrize("dtype", [G.F32, G.F64], ids=["fp32", "fp64"])
def test_minus_zero_is_not_plus_zero(dtype):
    whole, view = G.carve((3,), dtype, G.LEAD_ODD, 0, 8)
    off, size = G.span(whole, view)
    assert (whole == 0).all() and G.intact(whole, (off, size), 0).ok
    w = whole.copy()
    w[off - 1] = -0.0
    assert (w == 0).all() and G.intact(w, (off, size), 0) == (False, -1, 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_an_untouched_buffer_passes_and_a_copy_of_it_too(dtype):
    for kind in ("in", "out"):
        if kind == "in" and dtype == G.I32:
            continue
        fill = fill_of(dtype, kind)
        whole, view = G.carve((2, 9, 9), dtype, G.LEAD_ODD, fill, G.margin_for(9))
        view[...] = np.arange(162).reshape(2, 9, 9)
        sp = G.span(whole, view)
        assert G.intact(whole, sp, fill).ok and G.intact(whole.copy(), sp, fill).ok
        assert G.same_bits(whole, whole.copy()) and G.first_difference(whole, whole.copy()) is None


def test_the_fill_patterns_are_what_they_claim():
    for dt in (G.F32, G.F64):
        for table in (G.NAN_IN, G.SENTINEL):
            v = np.array([table[dt]], G.BITS[np.dtype(dt).itemsize]).view(dt)[0]
            assert np.isnan(v)
            assert table[dt] != G.bits_of(np.array([np.nan], dt))[0]       # not the NaN arithmetic produces
            assert table[dt] != G.bits_of(-np.array([np.nan], dt))[0]
        assert G.NAN_IN[dt] != G.SENTINEL[dt]
    s = np.array([G.SENTINEL[G.I32]], np.uint32).view(np.int32)[0]
    assert s > 3 and s > 2 ** 20                                          # no status word, no determinant exponent


def test_same_bits_is_strict():
    a = np.array([0.0, 1.0, np.nan], G.F32)
    b = a.copy()
    assert G.same_bits(a, b)
    b[0] = -0.0
    assert not G.same_bits(a, b) and G.first_difference(a, b)["first"] == 0
    assert not G.same_bits(a, a.astype(G.F64)) and not G.same_bits(a, a[:2])


def test_route_tables():
    names = [r.name for r in G.INV_ROUTES]
    assert len(set(names)) == len(names)
    by = {r.name: r for r in G.INV_ROUTES}
    assert by["wide"].orders == by["wide_nopivot"].orders == tuple(wide_cases.EDGE_ORDERS)
    assert by["blocked32"].orders == (16, 130, 256, 300) and by["blocked32"].batches == (1, 3)
    assert by["blocked64"].orders == (256, 300) and by["nopivot_blocked"].orders == (520, 640)
    assert G.DET_ORDERS == tuple(ovf.DET_ORDERS)
    assert set(G.RESIDUAL_ORDERS) <= set(residual_cases.FLOAT_ORDERS) and all(n % 64 for n in G.RESIDUAL_ORDERS)
    assert {n & 3 == 0 for n in G.RESIDUAL_ORDERS} == {True, False}
    assert G.SPLIT_BATCH * G.SPLIT_ORDER ** 2 == 64 * 1024 * 1024 and G.SPLIT_BATCH >= 4
    assert [G.tail_batch(l) for l in (8, 16, 32, 64)] == [33, 17, 9, 5]
