"""GPU test of the panel step at 1, 2, 3 and 4 rows per lane: pivoting inversions with exact ties in pivot columns
(two rows of one lane, of two lanes, of two waves) and with columns where no swap happens, bit for bit against the
oracle -- ties and no-swap steps are where the order of the label exchange and the winner's overwrite shows."""
import numpy as np
import pytest

from panel_tie_cases import CASES, oracle_inverse, tie_matrix

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gpu_matrix_inversion_amd as g  # noqa: E402


@pytest.mark.parametrize("n,deltas", CASES)
def test_ties_and_no_swap_columns_bit_identical_to_oracle(oracle, n, deltas):
    a, _ = tie_matrix(n, deltas, 77_000 + n)
    want, info = oracle_inverse(oracle, a, n)
    assert info["status"] == 0
    inv = g.Inverter(algo="blocked")
    try:
        x, st = inv.inv(torch.from_numpy(a).cuda())
        torch.cuda.synchronize()
        got, st = x.cpu().numpy(), st.cpu().numpy()
    finally:
        inv.close()
    assert st[0] == 0
    bad = np.argwhere(got.reshape(n, n) != want.reshape(n, n))
    assert len(bad) == 0, (len(bad), bad[:8].tolist())
