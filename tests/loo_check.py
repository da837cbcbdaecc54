"""Comparators of b9_filter_loo's outputs against tests/loo_ref.py, used by the GPU suite and by the CPU suite that checks the
comparators' own power (tests/test_filterloo_host.py).  The tolerances are resid_check's, derived there:

rtol 1e-9 plus two absolute terms per entry: the pruning's bound (N_nodes e^-40 times what one dropped unit of weight can
move the entry by -- loo_ref's `bound`; dropped with b9_tuning.marg_no_pruning) and rtol times the scale of the entry's
rounding (loo_ref's `absx`: p sum w^f |d_f| for a first moment, which cancels where the prediction straddles the observation;
p max(1, |L|, |L^f|) for p l_f, a difference of two log-sums).  The row columns get these bounds carried through their sums.
ROWS is compared exactly."""
import numpy as np

from resid_check import CUT, RTOL, largest_rel          # noqa: F401  (re-exported)


def star_atol(bound, absx, n_nodes, pruning=True):
    """[star, 2 + 3 nf] from loo_ref's per-row bound / absx [row, star, 2 + 3 nf]."""
    a = RTOL * np.asarray(absx).sum(axis=0)
    if pruning:
        a = a + n_nodes * CUT * np.asarray(bound).sum(axis=0)
    return a


def row_atol(bound, absx, sigma, n_nodes, pruning=True):
    """[row, 1 + 6 nf]: the per-(row, star) bounds carried through the row sums."""
    bound, absx = np.asarray(bound), np.asarray(absx)
    per = RTOL * absx + (n_nodes * CUT * bound if pruning else 0.0)          # [row, star, 2 + 3 nf]
    sig = np.asarray(sigma, dtype=np.float64)
    used = sig > 0
    s = np.where(used, 1.0 / np.where(used, sig, 1.0), 0.0)                  # [star, nf]
    n_rows, n, nc = per.shape
    nf = (nc - 2) // 3
    out = np.zeros((n_rows, 1 + 6 * nf))
    out[:, 0] = per[:, :, 1].sum(axis=1)
    for f in range(nf):
        u = used[:, f]
        out[:, 1 + 6 * f] = per[:, u, 1].sum(axis=1)
        out[:, 2 + 6 * f] = (per[:, :, 2 + 3 * f] * s[None, :, f]).sum(axis=1)
        out[:, 3 + 6 * f] = (per[:, :, 3 + 3 * f] * s[None, :, f] ** 2).sum(axis=1)
        out[:, 4 + 6 * f] = (per[:, :, 1] * s[None, :, f] ** 2).sum(axis=1)
        out[:, 5 + 6 * f] = (per[:, :, 2 + 3 * f] * s[None, :, f] ** 2).sum(axis=1)
        out[:, 6 + 6 * f] = per[:, u, 4 + 3 * f].sum(axis=1)
    return out


def assert_star_loo(got, want, atol):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert np.array_equal(got[:, 0], want[:, 0]), "ROWS"
    assert np.all(np.abs(got[:, 1:] - want[:, 1:]) <= RTOL * np.abs(want[:, 1:]) + atol[:, 1:]), "star_loo"


def assert_row_loo(got, want, atol):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert np.all(np.abs(got - want) <= RTOL * np.abs(want) + atol), "row_loo"


def star_moments_of(acc):
    """(mean d, second moment, variance), each [star, nf], of an accumulator; zeros without membership weight."""
    acc = np.asarray(acc, dtype=np.float64)
    m = acc[:, 1] > 0
    m1, m2 = np.zeros_like(acc[:, 2::3]), np.zeros_like(acc[:, 3::3])
    m1[m], m2[m] = acc[m, 2::3] / acc[m, 1:2], acc[m, 3::3] / acc[m, 1:2]
    return m1, m2, m2 - m1 ** 2


def assert_variances(got_acc, want_acc):
    """The between-node variances of the two accumulators, atol 1e-9 x the second moment (resid_check.assert_variances)."""
    _, m2, var_want = star_moments_of(want_acc)
    _, _, var_got = star_moments_of(got_acc)
    assert np.all(np.abs(var_got - var_want) <= RTOL * np.abs(m2)), "variances"


def assert_star_table(got, want, want_acc, cl):
    """Two per-star tables [star, 2 + 5 nf]: looMag and lpd at rtol, resid with looMag's absolute error (atol rtol |looMag|),
    looSd through its square with the variance's atol, z = resid / sqrt(sigma^2 + var) with both carried through."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert np.array_equal(got[:, 0], want[:, 0]), "rows"
    np.testing.assert_allclose(got[:, 1], want[:, 1], rtol=RTOL, atol=1e-300, err_msg="member")
    _, m2, _ = star_moments_of(want_acc)
    sig = np.asarray(cl["sigma"], dtype=np.float64)
    pred = np.abs(want[:, 2::5])
    np.testing.assert_allclose(got[:, 2::5], want[:, 2::5], rtol=RTOL, atol=0, err_msg="looMag")
    assert np.all(np.abs(got[:, 3::5] ** 2 - want[:, 3::5] ** 2) <= RTOL * np.abs(m2)), "looSd"
    resid_tol = RTOL * (np.abs(want[:, 4::5]) + pred)
    assert np.all(np.abs(got[:, 4::5] - want[:, 4::5]) <= resid_tol), "resid"
    # z = resid / s, s^2 = sigma^2 + var: |dz| <= |d resid| / s + |z| |d var| / (2 s^2)
    s2 = np.where(sig > 0, sig, 1.0) ** 2 + want[:, 3::5] ** 2
    z_tol = resid_tol / np.sqrt(s2) + np.abs(want[:, 5::5]) * RTOL * np.abs(m2) / (2 * s2) + RTOL * np.abs(want[:, 5::5])
    assert np.all(np.abs(got[:, 5::5] - want[:, 5::5]) <= z_tol), "z"
    np.testing.assert_allclose(got[:, 6::5], want[:, 6::5], rtol=RTOL, atol=0, err_msg="lpd")


def assert_filter_table(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert np.array_equal(got[:, 0], want[:, 0]), "nRows"
    # resid_check.assert_filter_table's reasoning, four quantities: 4 rtol x the quantity's largest statistic + sd
    scale = np.repeat(np.stack([np.abs(want[:, 1 + 5 * k:6 + 5 * k]).max(axis=1) + want[:, 2 + 5 * k] for k in range(4)], axis=1), 5, axis=1)
    assert np.all(np.abs(got[:, 1:] - want[:, 1:]) <= 4 * RTOL * scale), "filter table"
