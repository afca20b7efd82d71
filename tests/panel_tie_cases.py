"""Inputs for the panel-step tests: inversions whose pivot search meets exact ties, and columns without a swap.

tie_matrix(n, deltas, seed): U(-1,1) + sqrt(n) I with a quarter of the rows swapped in pairs (so the matrix has both
steps that swap and steps that do not), and pairs of "tie rows": both rows of a pair are zero in every column before
column j and hold the same large |v| in column j.  A row whose entries in the earlier pivot columns are zero has zero
multipliers in those steps, so fmaf(-0, u, x) leaves it exactly as it is: when step j runs, the two rows still hold
+-v, far above every other entry of the column, and the search has to break an exact tie by position.

In the first sub-panel of the first block the panel holds the rows in input order (register row k of thread t: row
V t + k with V consecutive rows per lane, or k NT + t at three rows per lane), so the pairs of columns 0, 1, 2 are
placed on purpose, `deltas` apart: two rows of one lane (adjacent lanes at one row per lane), two lanes of one wave,
two waves.  The pairs at later columns (other sub-panels, the second block) meet whatever lanes hold them by then.
"""
import numpy as np

TIE_VALUE = 4096.0


def tie_columns(n):
    return [j for j in (0, 1, 2, 7, 15, 17, 33, 130, 300) if j < n // 2]


def tie_matrix(n, deltas, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, (n, n)) + np.sqrt(n) * np.eye(n)
    # swap a quarter of the rows in pairs: those columns' steps exchange two rows, the others' do not
    idx = rng.permutation(n)[: (n // 4) & ~1].reshape(-1, 2)
    a[np.concatenate([idx[:, 0], idx[:, 1]])] = a[np.concatenate([idx[:, 1], idx[:, 0]])]
    base = (n // 2) & ~3
    used = set()
    pairs = {}
    for j in tie_columns(n):
        if j < 3:
            r1, r2 = base + 16 * j, base + 16 * j + deltas[j]
        else:
            while True:
                r1, r2 = (int(v) for v in rng.integers(j + 1, n, 2))
                if r1 != r2 and not {r1, r2} & (used | set(range(base, base + 1100))):
                    break
        assert 0 <= r1 < n and 0 <= r2 < n and not {r1, r2} & used, (j, r1, r2)
        used |= {r1, r2}
        pairs[j] = (r1, r2)
        for r, sign in ((r1, 1.0), (r2, -1.0 if j % 2 else 1.0)):
            a[r] = rng.uniform(-1.0, 1.0, n)
            a[r, :j] = 0.0
            a[r, j] = sign * TIE_VALUE
    return a.astype(np.float32), pairs


def oracle_inverse(oracle, a, n):
    """(result, info) of the reference-order oracle: step by step up to 1024, its cache-blocked evaluation above."""
    if n <= 1024:
        return oracle.matrix_inv_32_inplace(a, n, return_info=True)
    return oracle.matrix_inv_32_blocked_exact(a, n, 128, return_info=True)


# (n, row distances of the pairs in columns 0, 1, 2): the first panel of each runs at 1, 2, 3 and 4 rows per lane
# (512 x 1, 1024 x 2, 1024 x 3, 1024 x 4)
CASES = [(500, (1, 8, 64)), (2048, (1, 8, 128)), (2560, (1024, 8, 64)), (3200, (1, 8, 256))]
