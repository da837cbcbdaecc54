"""Comparators of the b9_pointwise tests (tests only), shared by the CPU and the GPU suite.

Tolerances.  v, VMAX, RMAX, lppd = VMAX + log SPOS, elpdIs' RMAX + log SNEG, MEAN and row_lpd / n_stars are values of the size of
a star's log-likelihood: |delta| <= 1e-9 max(1, |value|), the project tolerance.  M2 = sum (v - mean)^2
is a difference of such values: with every v perturbed by at most delta = 1e-9 max(1, max |v|), each deviation moves by at most
2 delta, so |delta M2| <= sum (4 delta |v - mean| + 4 delta^2) <= 4 delta sqrt(n M2) + 4 n delta^2 (Cauchy-Schwarz).  The
pruning drops at most N_nodes e^-40 of a star's sum, 3e-15 relative on these grids: inside the tolerance.  Counts are exact;
-inf must sit where the reference has it."""
import numpy as np

import pointwise_ref as pr

TOL = 1e-9


def _close(got, want, what, tol=TOL):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} against {want.shape}"
    inf = ~np.isfinite(want)
    assert np.array_equal(got[inf], want[inf], equal_nan=True), f"{what}: the non-finite entries differ"
    err = np.abs(got[~inf] - want[~inf])
    bound = tol * np.maximum(1.0, np.abs(want[~inf]))
    assert np.all(err <= bound), f"{what}: largest |delta| / bound {np.max(err / bound):.3g}"


def largest(got, want):
    """largest |delta| / max(1, |want|) over the entries where both are finite"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    ok = np.isfinite(want) & np.isfinite(got)
    return float(np.max(np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok])))) if ok.any() else 0.0


def assert_values(got, want):
    _close(got, want, "v")


def assert_acc(got, want):
    got, want = np.asarray(got, dtype=np.float64).reshape(-1, pr.N), np.asarray(want, dtype=np.float64).reshape(-1, pr.N)
    assert np.array_equal(got[:, pr.ROWS], want[:, pr.ROWS]), "ROWS"
    assert np.array_equal(got[:, pr.NINF], want[:, pr.NINF]), "NINF"
    live = want[:, pr.ROWS] - want[:, pr.NINF] > 0
    assert np.all(got[~live, pr.VMAX:] == want[~live, pr.VMAX:]), "an empty star's finite columns must stay as they were"
    g, w = got[live], want[live]
    _close(g[:, pr.VMAX], w[:, pr.VMAX], "VMAX")
    _close(g[:, pr.RMAX], w[:, pr.RMAX], "RMAX")
    assert np.all(g[:, pr.SPOS] >= 1.0) and np.all(g[:, pr.SNEG] >= 1.0), "SPOS / SNEG hold the term of the maximum"
    _close(g[:, pr.VMAX] + np.log(g[:, pr.SPOS]), w[:, pr.VMAX] + np.log(w[:, pr.SPOS]), "VMAX + log SPOS")
    _close(g[:, pr.RMAX] + np.log(g[:, pr.SNEG]), w[:, pr.RMAX] + np.log(w[:, pr.SNEG]), "RMAX + log SNEG")
    _close(g[:, pr.MEAN], w[:, pr.MEAN], "MEAN")
    n = w[:, pr.ROWS] - w[:, pr.NINF]
    delta = TOL * np.maximum(1.0, np.maximum(np.abs(w[:, pr.VMAX]), np.abs(w[:, pr.RMAX])))
    bound = 4 * delta * np.sqrt(n * w[:, pr.M2]) + 4 * n * delta ** 2
    err = np.abs(g[:, pr.M2] - w[:, pr.M2])
    assert np.all(err <= bound), f"M2: largest |delta| / bound {np.max(err / bound):.3g}"


def assert_tail(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.all(got[:, :-1] >= got[:, 1:]), "the tail must descend"
    _close(got, want, "tail")


def assert_rows(got, want, n_stars):
    _close(np.asarray(got) / n_stars, np.asarray(want) / n_stars, "row_lpd / n_stars")


def assert_table(got, want, tol=TOL, loo_tol=None):
    """A per-star table against the reference's: counts exact, every other column at tol (elpdLoo and pLoo at loo_tol)."""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1, 9), np.asarray(want, dtype=np.float64).reshape(-1, 9)
    assert np.array_equal(got[:, :2], want[:, :2]), "rows / nInf"
    for c, name in ((pr.T_LPPD, "lppd"), (pr.T_PWAIC, "pWaic"), (pr.T_ELPD_WAIC, "elpdWaic"), (pr.T_ELPD_IS, "elpdIs"), (pr.T_K, "paretoK")):
        _close(got[:, c], want[:, c], name, tol)
    for c, name in ((pr.T_ELPD_LOO, "elpdLoo"), (pr.T_PLOO, "pLoo")):
        _close(got[:, c], want[:, c], name, loo_tol or tol)


def non_vacuity(acc, cl, live):
    """(stars with M2 > 0, live WD-stage stars) of a reference accumulator; live [row, star]."""
    from base_amd import abi
    acc = np.asarray(acc)
    wd = np.asarray(cl["stage"]) == abi.STAGE_WD
    return int((acc[:, pr.M2] > 0).sum()), int((wd & np.asarray(live).any(axis=0)).sum())
