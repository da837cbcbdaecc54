"""Comparators of b9_star_offset's outputs against tests/offset_ref.py, used by the GPU suite and by the CPU suite that checks
the comparators' own power (tests/test_offset_host.py).  They take the form of loo_check's, with resid_check's constants and no
new ones:

rtol 1e-9 plus two absolute terms per entry: the pruning's bound (N_nodes e^-40 times what one dropped unit of weight can
move the entry by -- offset_ref's `bound`: max |mu| and max mu^2 over the star's nodes for the two sums, |logBF| + 2 for the
last column; dropped with b9_tuning.marg_no_pruning) and rtol times the scale of the entry's rounding (offset_ref's `absx`:
p sum w' |mu| for the first moment, which cancels where the nodes' offsets straddle zero; p max(1, |L|, |L'|) for the log Bayes
factor, a difference of two log-sums).  The row columns get these bounds carried through their sums.  ROWS is compared exactly."""
import numpy as np

from resid_check import CUT, RTOL, largest_rel          # noqa: F401  (re-exported)


def star_atol(bound, absx, n_nodes, pruning=True):
    """[star, 2 + 3 D] from offset_ref's per-row bound / absx [row, star, 2 + 3 D]."""
    a = RTOL * np.asarray(absx).sum(axis=0)
    if pruning:
        a = a + n_nodes * CUT * np.asarray(bound).sum(axis=0)
    return a


def row_atol(bound, absx, C, V, n_nodes, pruning=True):
    """[row, 1 + 4 D]: the per-(row, star) bounds carried through the row sums; C, V [star, D] (offset_ref.all_cv)."""
    bound, absx = np.asarray(bound), np.asarray(absx)
    per = RTOL * absx + (n_nodes * CUT * bound if pruning else 0.0)          # [row, star, 2 + 3 D]
    n_rows, n, nc = per.shape
    nd = (nc - 2) // 3
    out = np.zeros((n_rows, 1 + 4 * nd))
    out[:, 0] = per[:, :, 1].sum(axis=1)
    for j in range(nd):
        u = np.asarray(C)[:, j] > 0
        out[:, 1 + 4 * j] = per[:, u, 1].sum(axis=1)
        out[:, 2 + 4 * j] = per[:, u, 2 + 3 * j].sum(axis=1)
        out[:, 3 + 4 * j] = (per[:, u, 3 + 3 * j] + per[:, u, 1] * np.asarray(V)[None, u, j]).sum(axis=1)
        out[:, 4 + 4 * j] = per[:, u, 4 + 3 * j].sum(axis=1)
    return out


def assert_star_off(got, want, atol):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert np.array_equal(got[:, 0], want[:, 0]), "ROWS"
    assert np.all(np.abs(got[:, 1:] - want[:, 1:]) <= RTOL * np.abs(want[:, 1:]) + atol[:, 1:]), "star_off"


def assert_row_off(got, want, atol):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert np.all(np.abs(got - want) <= RTOL * np.abs(want) + atol), "row_off"


def assert_star_table(got, want):
    """Two per-star tables [star, 2 + 4 D] formed from the SAME accumulator: rows exactly, the rest at rtol."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert np.array_equal(got[:, 0], want[:, 0]), "rows"
    np.testing.assert_allclose(got[:, 1:], want[:, 1:], rtol=RTOL, atol=1e-300, err_msg="star table")


def assert_dist_table(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert np.array_equal(got[:, 0], want[:, 0]), "nRows"
    # resid_check.assert_filter_table's reasoning, three quantities: 4 rtol x the quantity's largest statistic + sd
    scale = np.repeat(np.stack([np.abs(want[:, 1 + 5 * q:6 + 5 * q]).max(axis=1) + want[:, 2 + 5 * q] for q in range(3)], axis=1), 5, axis=1)
    assert np.all(np.abs(got[:, 1:] - want[:, 1:]) <= 4 * RTOL * scale), "dist table"
