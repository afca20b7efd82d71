"""Every dense route enqueues exactly the launches it did before the dense calls were planned in one place.

Launches are counted per kernel class with ``Inverter.set_profiling(True)`` / ``get_profile()`` on the smallest shapes
that reach each route, through ``inv``, ``inv_det_any`` and ``inv_det_any(want_inverse=False)`` (the two one-launch
shapes through ``inv_det`` as well).  EXPECTED was recorded once on an MI355X from a build of the commit PARENT -- the
parent of the change that introduced the DenseRoute -- by running ``launch_counts`` below against that build's library,
never from the code under test.  The status and output bytes of ``inv`` and ``inv_det_any`` agree for every shape.
The split-batch and look-ahead routes are too large for this file: test_gpu_sequences and test_gpu_det_large cover them.
"""
import numpy as np
import pytest

PARENT = "fb893b996147b6d5ce5e136d98f4b58d54ebb04f"

# id: (dtype, n, batch, Inverter arguments)
SHAPES = {
    "f32_sweep_n20_b3": ("float32", 20, 3, {}),
    "f32_blocked_n130_b1": ("float32", 130, 1, {}),
    "f32_blocked_n130_b2": ("float32", 130, 2, {}),
    "f32_blocked_n300_b1": ("float32", 300, 1, {}),
    "f32_blocked_n300_b2": ("float32", 300, 2, {}),
    "f32_nopivot_sweep_n300": ("float32", 300, 1, {"pivoting": False}),
    "f32_nopivot_blocked_n520": ("float32", 520, 1, {"pivoting": False}),
    "f64_sweep_n100": ("float64", 100, 1, {}),
    "f64_blocked_n260_bw64": ("float64", 260, 1, {"block_width": 64}),
    "f64_blocked_n260_bw128": ("float64", 260, 1, {"block_width": 128}),
    "f64_nopivot_sweep_n300": ("float64", 300, 1, {"pivoting": False}),
    "f64_nopivot_blocked_n520": ("float64", 520, 1, {"pivoting": False}),
    "resident_n8_b100": ("float32", 8, 100, {"algo": "resident"}),
    "workgroup_n100_b10": ("float32", 100, 10, {"algo": "workgroup"}),
}
ONE_LAUNCH = ("resident_n8_b100", "workgroup_n100_b10")  # these also run through inv_det


def _above_128(plain, finish_det, finish_det_only):
    """A route above order 128: the det calls enqueue the plain call's launches and differ in the finish class alone
    (input scan, pivot gathers or copies, parity, the det finish kernel; no un-permutation without the inverse)."""
    return {"inv": plain, "inv_det_any": {**plain, "finish": finish_det},
            "inv_det_any_no_inverse": {**plain, "finish": finish_det_only}}


def _one_launch(inv, calls=("inv_det_any", "inv_det_any_no_inverse")):
    """Up to order 128 every det call is one launch of a one-launch kernel (the panel class), whatever ``inv`` runs."""
    return {"inv": inv, **{c: {"panel": 1} for c in calls}}


_SWEEP300 = {"init": 1, "sweep_step": 300, "finish": 1}
_F32_N130 = {"init": 1, "panel": 16, "update_in_block": 1, "finish": 1}
_F32_N300 = {"init": 1, "panel": 24, "update_in_block": 2, "update_rank_bw": 2, "finish": 1, "panel_transpose": 2}
_ALL_DET = ("inv_det_any", "inv_det_any_no_inverse", "inv_det", "inv_det_no_inverse")
# {shape: {call: {kernel class: launches}}}, classes without a launch left out; recorded from PARENT
EXPECTED = {
    "f32_sweep_n20_b3": _one_launch({"init": 1, "sweep_step": 20, "finish": 1}),
    "f32_blocked_n130_b1": _above_128(_F32_N130, 4, 4),
    "f32_blocked_n130_b2": _above_128(_F32_N130, 4, 4),
    "f32_blocked_n300_b1": _above_128(_F32_N300, 5, 5),
    "f32_blocked_n300_b2": _above_128(_F32_N300, 5, 5),
    "f32_nopivot_sweep_n300": _above_128(_SWEEP300, 3, 2),
    "f32_nopivot_blocked_n520": _above_128({"init": 1, "panel": 40, "update_in_block": 40, "update_rank_bw": 3, "finish": 1,
                                            "panel_transpose": 3}, 6, 6),
    "f64_sweep_n100": _one_launch({"init": 1, "sweep_step": 100, "finish": 1}),
    "f64_blocked_n260_bw64": _above_128({"init": 1, "panel": 325, "update_rank_bw": 5, "finish": 1}, 3, 2),
    "f64_blocked_n260_bw128": _above_128({"init": 1, "panel": 387, "update_rank_bw": 3, "finish": 1}, 3, 2),
    "f64_nopivot_sweep_n300": _above_128(_SWEEP300, 3, 2),
    "f64_nopivot_blocked_n520": _above_128({"init": 1, "panel": 9, "update_in_block": 9, "update_rank_bw": 9, "finish": 1},
                                           12, 11),
    "resident_n8_b100": _one_launch({"panel": 1}, _ALL_DET),
    "workgroup_n100_b10": _one_launch({"panel": 1}, _ALL_DET),
}


def dominant(n, batch, dtype, seed):
    """Strictly diagonally dominant members: every path inverts them, the no-pivot ones included."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, (batch, n, n))
    a[:, np.arange(n), np.arange(n)] = np.abs(a).sum(axis=2) + 1.0
    return a.astype(dtype)


def calls_of(shape):
    calls = {"inv": lambda inv, a: inv.inv(a),
             "inv_det_any": lambda inv, a: inv.inv_det_any(a),
             "inv_det_any_no_inverse": lambda inv, a: inv.inv_det_any(a, want_inverse=False)}
    if shape in ONE_LAUNCH:
        calls["inv_det"] = lambda inv, a: inv.inv_det(a)
        calls["inv_det_no_inverse"] = lambda inv, a: inv.inv_det(a, want_inverse=False)
    return calls


def launch_counts(shape):
    """``({call: {kernel class: launches}}, {call: what the call returned, on the host})`` of one shape."""
    import torch

    import gpu_matrix_inversion_amd as g

    dtype, n, batch, kwargs = SHAPES[shape]
    a = torch.from_numpy(dominant(n, batch, dtype, 1000 + n)).cuda()
    inv = g.Inverter(**kwargs)
    counts, results = {}, {}
    try:
        inv.set_profiling(True)
        for name, call in calls_of(shape).items():
            inv.get_profile()  # drop what the call before left
            out = call(inv, a)
            counts[name] = {k: c for k, (_, c) in inv.get_profile().items() if c}
            results[name] = [None if t is None else t.cpu().numpy() for t in out]
        inv.set_profiling(False)
    finally:
        inv.close()
    return counts, results


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_launches_per_kernel_class_are_the_parents(shape):
    counts, results = launch_counts(shape)
    assert counts == EXPECTED[shape]
    x, st = results["inv"]
    assert not st.any()
    for name, got in results.items():
        if name == "inv":
            continue
        assert got[1].tobytes() == st.tobytes(), name
        if name.endswith("no_inverse"):
            assert got[0] is None, name
        else:
            assert got[0].tobytes() == x.tobytes(), name
        assert np.isfinite(got[2]).all() and (np.abs(got[2]) >= 0.5).all() and (np.abs(got[2]) < 1.0).all(), name
    # the determinant does not depend on whether the inverse is stored
    assert results["inv_det_any"][2].tobytes() == results["inv_det_any_no_inverse"][2].tobytes()
    assert results["inv_det_any"][3].tobytes() == results["inv_det_any_no_inverse"][3].tobytes()
