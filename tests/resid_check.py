"""Comparators of b9_phot_resid's outputs against tests/resid_ref.py, used by the GPU suite and by the CPU suite that checks
the comparators' own power (tests/test_resid_host.py).  The tolerances are derived, not fitted:

rtol 1e-9 -- the project's per-star tolerance -- plus two absolute terms per entry.

Pruning.  The kernels may drop terms more than 40 e-folds below a lower bound of the star's largest: each dropped node
weighs < e^-40, at most N_nodes of them (the nodes of a star's grid, all populations).  Per row that moves MEMBER by at most
N_nodes e^-40, column 2 + 2f by N_nodes e^-40 max |d_f| and column 3 + 2f by N_nodes e^-40 max d_f^2, the maxima over the
star's nodes in the reference (resid_ref's `bound`); an accumulator entry sums its rows' bounds.  The row columns get these
bounds carried through their sums: col 0 and N_f sum the stars' MEMBER bounds, R_f the first-moment bounds / sigma, C_f the
second-moment bounds / sigma^2, W_f the MEMBER bounds / sigma^2, D_f the first-moment bounds / sigma^2.

Zeros.  A first-moment column p sum w d_f cancels where the posterior straddles the observation, so an entry can be
arbitrarily small next to its terms; the rounding of any summation order scales with p sum w |d_f| (resid_ref's `absx`), and
rtol times that is the entry's second absolute term (for every other column absx = |x| and the term adds nothing new).
With pruning off (b9_tuning.marg_no_pruning) the first term is dropped: what is left separates pruning from arithmetic.

ROWS is compared exactly.  Variances are compared as variances, with an atol of 1e-9 times the second moment they were formed
from, not as standard deviations."""
import numpy as np

RTOL = 1e-9
CUT = np.exp(-40.0)


def star_atol(bound, absx, n_nodes, pruning=True):
    """[star, 2 + 2 nf] from resid_ref's per-row bound / absx [row, star, 2 + 2 nf]."""
    a = RTOL * np.asarray(absx).sum(axis=0)
    if pruning:
        a = a + n_nodes * CUT * np.asarray(bound).sum(axis=0)
    return a


def row_atol(bound, absx, sigma, n_nodes, pruning=True):
    """[row, 1 + 5 nf]: the per-(row, star) bounds carried through the row sums."""
    bound, absx = np.asarray(bound), np.asarray(absx)
    per = RTOL * absx + (n_nodes * CUT * bound if pruning else 0.0)          # [row, star, 2 + 2 nf]
    sig = np.asarray(sigma, dtype=np.float64)
    used = sig > 0
    s = np.where(used, 1.0 / np.where(used, sig, 1.0), 0.0)                  # [star, nf]
    n_rows, n, nc = per.shape
    nf = (nc - 2) // 2
    out = np.zeros((n_rows, 1 + 5 * nf))
    out[:, 0] = per[:, :, 1].sum(axis=1)
    for f in range(nf):
        u = used[:, f]
        out[:, 1 + 5 * f] = per[:, u, 1].sum(axis=1)
        out[:, 2 + 5 * f] = (per[:, :, 2 + 2 * f] * s[None, :, f]).sum(axis=1)
        out[:, 3 + 5 * f] = (per[:, :, 3 + 2 * f] * s[None, :, f] ** 2).sum(axis=1)
        out[:, 4 + 5 * f] = (per[:, :, 1] * s[None, :, f] ** 2).sum(axis=1)
        out[:, 5 + 5 * f] = (per[:, :, 2 + 2 * f] * s[None, :, f] ** 2).sum(axis=1)
    return out


def largest_rel(got, want, floor=1e-6):
    """The largest relative difference among the entries above `floor`."""
    got, want = np.asarray(got), np.asarray(want)
    nz = np.abs(want) > floor
    return float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz]))) if nz.any() else 0.0


def assert_star_resid(got, want, atol):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert np.array_equal(got[:, 0], want[:, 0]), "ROWS"
    assert np.all(np.abs(got[:, 1:] - want[:, 1:]) <= RTOL * np.abs(want[:, 1:]) + atol[:, 1:]), "star_resid"


def assert_row_resid(got, want, atol):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert np.all(np.abs(got - want) <= RTOL * np.abs(want) + atol), "row_resid"


def assert_variances(got_acc, want_acc, cl):
    """The variances acc[3+2f] / acc[1] - (acc[2+2f] / acc[1])^2 of the two accumulators, atol 1e-9 x the second moment."""
    import resid_ref as rr
    _, m2, var_want = rr.star_moments_of(want_acc, cl)
    _, _, var_got = rr.star_moments_of(got_acc, cl)
    assert np.all(np.abs(var_got - var_want) <= RTOL * np.abs(m2)), "variances"


def assert_star_table(got, want, want_acc, cl):
    """Two per-star tables [star, 2 + 4 nf]: predMag, resid and rmsZ at rtol (resid carries predMag's absolute error: atol
    rtol |predMag|), predSd through its square with the variance's atol."""
    import resid_ref as rr
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert np.array_equal(got[:, 0], want[:, 0]), "rows"
    np.testing.assert_allclose(got[:, 1], want[:, 1], rtol=RTOL, atol=1e-300, err_msg="member")
    _, m2, _ = rr.star_moments_of(want_acc, cl)
    pred = np.abs(want[:, 2::4])
    np.testing.assert_allclose(got[:, 2::4], want[:, 2::4], rtol=RTOL, atol=0, err_msg="predMag")
    assert np.all(np.abs(got[:, 3::4] ** 2 - want[:, 3::4] ** 2) <= RTOL * np.abs(m2)), "predSd"
    assert np.all(np.abs(got[:, 4::4] - want[:, 4::4]) <= RTOL * (np.abs(want[:, 4::4]) + pred)), "resid"
    np.testing.assert_allclose(got[:, 5::4], want[:, 5::4], rtol=RTOL, atol=0, err_msg="rmsZ")


def assert_filter_table(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert np.array_equal(got[:, 0], want[:, 0]), "nRows"
    # a row's ratio of two sums that meet rtol is within 2 rtol of itself; a mean or a percentile of such values moves by no
    # more than the largest of them does, a standard deviation by twice that: 4 rtol x the quantity's largest statistic + sd
    scale = np.repeat(np.stack([np.abs(want[:, 1 + 5 * k:6 + 5 * k]).max(axis=1) + want[:, 2 + 5 * k] for k in range(3)], axis=1), 5, axis=1)
    assert np.all(np.abs(got[:, 1:] - want[:, 1:]) <= 4 * RTOL * scale), "filter table"


def non_vacuity(want_acc, cl):
    """(live stars, live stars with predSd > 1e-6 in some filter, stars with an unused filter, WD-stage stars with member > 0)
    of a reference accumulator."""
    import resid_ref as rr
    from base_amd import abi
    tab = rr.star_table(want_acc, cl)
    live = np.asarray(want_acc)[:, 1] > 0
    spread = (tab[:, 3::4] > 1e-6).any(axis=1) & live
    unused = (~(np.asarray(cl["sigma"]) > 0)).any(axis=1)
    wd = (np.asarray(cl["stage"]) == abi.STAGE_WD) & live
    return int(live.sum()), int(spread.sum()), int(unused.sum()), int(wd.sum())
