"""Comparators of the b9_star_influence tests (tests only), shared by the CPU and the GPU suite.

Tolerances, from the project tolerance as pointwise_check.py derives M2's.  Every v is right to
delta = 1e-9 max(1, max |v|) of its star.  RMAX, RMAX + log SNEG and MEANV are values of the size of a log-likelihood: the
project tolerance itself.  A weight w = e^(-v - RMAX) has both v and RMAX moved by at most delta, so it is off by at most
e^(2 delta) - 1 <= 2 delta (1 + 2 delta) relatively, and w^2 by twice that:
    |d SNEG|  <= 2 delta SNEG,       |d SNEG2| <= 4 delta SNEG2,
    |d WQ_j|  <= 2 delta sum w |q_j|,  |d WQ2_j| <= 2 delta sum w q_j^2,
each with the factor (1 + 2 delta) and, for the rounding of at most n terms, n 2^-52 of the same sum of magnitudes.  MQ does not
depend on v: n 2^-52 max |q| of rounding (a Welford step rounds thrice).  CVQ = sum (v - mean v)(q - mean q): every deviation of
v moves by at most 2 delta, so |d CVQ| <= 2 delta sum |q - mean q| plus the rounding 4 n 2^-52 sum |v - mean v| |q - mean q|.
The table's columns follow: m = WQ / SNEG moves by at most dm = 4 delta' sum w |q| / SNEG (numerator and denominator, delta' =
delta (1 + 2 delta) + n 2^-52), shift = m - MQ by that plus MQ's rounding; var = WQ2 / SNEG - m^2 by
dvar = 4 delta' WQ2 / SNEG + 2 |m| dm + dm^2, and looSd = sqrt(var) by at most min(sqrt(dvar), dvar / looSd); lin = -CVQ / (n - 1)
by CVQ's bound over n - 1; ess = SNEG^2 / SNEG2 by 8 delta' relatively.  paretoK is compared at the project tolerance, as
pointwise_check does.  A group's sum over n_g stars is right to n_g delta (pointwise_check.assert_rows' rule).  Counts are exact;
NaN and -inf must sit where the reference has them."""
import numpy as np

import influence_ref as ir

TOL = 1e-9
EPS = 2.0 ** -52


def _bounded(got, want, bound, what):
    got, want, bound = (np.asarray(x, dtype=np.float64) for x in (got, want, bound))
    assert got.shape == want.shape, f"{what}: shape {got.shape} against {want.shape}"
    odd = ~np.isfinite(want)
    assert np.array_equal(got[odd], want[odd], equal_nan=True), f"{what}: the non-finite entries differ"
    err = np.abs(got[~odd] - want[~odd])
    b = np.broadcast_to(bound, want.shape)[~odd]
    assert np.all(err <= b), f"{what}: largest |delta| / bound {np.max(err / np.maximum(b, 1e-300)):.3g}"


def _close(got, want, what, tol=TOL):
    want = np.asarray(want, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        _bounded(got, want, tol * np.maximum(1.0, np.abs(np.where(np.isfinite(want), want, 0.0))), what)


def scales(V, inside, q):
    """Per star what the bounds are stated on: (delta' [star], n [star], mag [star, 2 + 3 Q] -- influence_ref.direct's sums of
    magnitudes --, qmax)."""
    V = np.asarray(V, dtype=np.float64)
    inside = np.ones(len(V), bool) if inside is None else np.asarray(inside, bool)
    _, mag = ir.direct(V, inside, q)
    Vi = V[inside]
    fin = np.isfinite(Vi)
    n = fin.sum(axis=0).astype(np.float64)
    vmax = np.max(np.where(fin, np.abs(Vi), 0.0), axis=0) if len(Vi) else np.zeros(V.shape[1])
    delta = TOL * np.maximum(1.0, vmax)
    return delta * (1 + 2 * delta) + n * EPS, n, mag, float(np.max(np.abs(q))) if np.size(q) else 0.0


def assert_acc(got, want, V, inside, q):
    """A state [star, 6 + 4 Q] against the reference's, on the values V [row, star] both were formed from (to the tolerance)."""
    q = np.asarray(q, dtype=np.float64).reshape(len(V), -1)
    Q = q.shape[1]
    got, want = np.asarray(got, dtype=np.float64).reshape(-1, ir.N(Q)), np.asarray(want, dtype=np.float64).reshape(-1, ir.N(Q))
    assert np.array_equal(got[:, ir.ROWS], want[:, ir.ROWS]), "ROWS"
    assert np.array_equal(got[:, ir.NINF], want[:, ir.NINF]), "NINF"
    live = want[:, ir.ROWS] - want[:, ir.NINF] > 0
    assert np.all(got[~live, ir.RMAX:] == want[~live, ir.RMAX:]), "an empty star's finite columns must stay as they were"
    d, n, mag, qmax = scales(V, inside, q)
    d, n, mag, g, w = d[live], n[live], mag[live], got[live], want[live]
    _close(g[:, ir.RMAX], w[:, ir.RMAX], "RMAX")
    assert np.all(g[:, ir.SNEG] >= 1.0) and np.all(g[:, ir.SNEG2] >= 1.0), "SNEG / SNEG2 hold the term of the maximum"
    _close(g[:, ir.RMAX] + np.log(g[:, ir.SNEG]), w[:, ir.RMAX] + np.log(w[:, ir.SNEG]), "RMAX + log SNEG")
    _close(g[:, ir.MEANV], w[:, ir.MEANV], "MEANV")
    _bounded(g[:, ir.SNEG], w[:, ir.SNEG], 2 * d * w[:, ir.SNEG], "SNEG")
    _bounded(g[:, ir.SNEG2], w[:, ir.SNEG2], 4 * d * w[:, ir.SNEG2], "SNEG2")
    for j in range(Q):
        c, m = ir.WQ(j), mag[:, 2 + 3 * j:5 + 3 * j]
        _bounded(g[:, c], w[:, c], 2 * d * m[:, 0], f"WQ[{j}]")
        _bounded(g[:, c + 1], w[:, c + 1], 2 * d * m[:, 1], f"WQ2[{j}]")
        _bounded(g[:, c + 2], w[:, c + 2], 4 * n * EPS * max(1.0, qmax), f"MQ[{j}]")
        dev = np.array([np.sum(np.abs(q[np.asarray(inside, bool)][:, j] - mq)) for mq in w[:, c + 2]])      # (every star has the same finite rows here, or fewer)
        _bounded(g[:, c + 3], w[:, c + 3], 2 * d * dev + 4 * n * EPS * m[:, 2], f"CVQ[{j}]")


def assert_groups(got, want, V, inside, group):
    """group_lpd [row, group] against the reference's: a sum over n_g stars at n_g times the project tolerance."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    V = np.asarray(V, dtype=np.float64)
    for g in range(want.shape[1]):
        n_g = max(1, int(np.sum(np.asarray(group) == g)))
        _close(got[:, g] / n_g, want[:, g] / n_g, f"group_lpd[:, {g}] / n_g")


def assert_table(got, want, V, inside, q):
    """A per-star table [star, 4 + 3 Q] against the reference's."""
    q = np.asarray(q, dtype=np.float64).reshape(len(V), -1)
    Q = q.shape[1]
    got, want = np.asarray(got, dtype=np.float64).reshape(-1, ir.STAR_HEAD + 3 * Q), np.asarray(want, dtype=np.float64).reshape(-1, ir.STAR_HEAD + 3 * Q)
    assert np.array_equal(got[:, :2], want[:, :2]), "rows / nInf"
    d, n, mag, qmax = scales(V, inside, q)
    _bounded(got[:, 2], want[:, 2], 8 * d * np.where(np.isfinite(want[:, 2]), want[:, 2], 0.0), "ess")
    _close(got[:, 3], want[:, 3], "paretoK")
    sneg = np.maximum(mag[:, 0], 1.0)
    qi = q[np.asarray(inside, bool)] if inside is not None else q
    for j in range(Q):
        c, m = ir.STAR_HEAD + 3 * j, mag[:, 2 + 3 * j:5 + 3 * j]
        dm = 4 * d * m[:, 0] / sneg
        _bounded(got[:, c], want[:, c], dm + 4 * n * EPS * max(1.0, qmax), f"shift[{j}]")
        dev = float(np.sum(np.abs(qi[:, j] - qi[:, j].mean()))) if len(qi) else 0.0
        _bounded(got[:, c + 1], want[:, c + 1], (2 * d * dev + 4 * n * EPS * m[:, 2]) / np.maximum(n - 1, 1), f"lin[{j}]")
        mean = m[:, 0] / sneg                                # >= |WQ / SNEG|
        dvar = 4 * d * m[:, 1] / sneg + 2 * mean * dm + dm * dm
        sd = np.where(np.isfinite(want[:, c + 2]), want[:, c + 2], 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            _bounded(got[:, c + 2], want[:, c + 2], np.minimum(np.sqrt(dvar), np.where(sd > 0, dvar / sd, np.inf)), f"looSd[{j}]")


def assert_group_table(got, want, tol=TOL):
    """A per-group table against the reference's formed from the SAME group_lpd: host arithmetic on identical input, held to the
    project tolerance; counts exact."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    assert np.array_equal(got[:, :3], want[:, :3]), "nStars / rows / nInf"
    _close(got[:, 3:], want[:, 3:], "the group table", tol)


def non_vacuity(acc, shift, cl, live, group):
    """(stars with SNEG > 1 and a non-zero shift, live WD-stage stars, stars per group) of a reference state and table."""
    from base_amd import abi
    wd = np.asarray(cl["stage"]) == abi.STAGE_WD
    moved = (np.asarray(acc)[:, ir.SNEG] > 1) & (np.asarray(shift) != 0).all(axis=1)
    return int(moved.sum()), int((wd & np.asarray(live).any(axis=0)).sum()), np.bincount(np.asarray(group)[np.asarray(group) >= 0])
