"""The comparators of b9_cmd_band against tests/band_ref.py, shared by the CPU tests (tests/test_cmdband_host.py: every
comparator rejects the reference's faulty stand-ins) and the GPU tests (tests/test_gpu_cmdband.py).

Tolerances.  MAG_TOL = 1e-10 mag is what tests/test_gpu_sim.py holds b9_predict_mags to against the same numpy forward model; a
line's MIN and MAX are single values, SUM is N of them about the pivot, SUMSQ N squares of them.  The mass columns and the
single-star magnitudes are copies of the oracle's isochrone plus one add: bit for bit -- and since the accumulation is one plain
IEEE operation per row in ascending row order on both sides, so are all five moments of those lines, given the same pivots."""
import math

import numpy as np

import band_ref as br

MAG_TOL = 1e-10
EDGE_MARGIN = 1e-9


def rejects(check, *args, **kw):
    try:
        check(*args, **kw)
    except AssertionError:
        return True
    return False


def exact_lines(spec, n_filt, n_pops):
    """[n_lines] bool: the lines whose values are copies (mass columns; the magnitude columns of the q = 0 loci)"""
    P, C, n_lines = br.shape_of(spec, n_filt, n_pops)
    ex = np.zeros(n_lines, dtype=bool)
    ex.reshape(n_pops * P, C)[:, 0] = True
    for k in range(n_pops):
        for s, q in enumerate(spec.ratios):
            if q == 0.0:
                for e in range(spec.n_eep):
                    o = br.line_index(spec, n_filt, k, s * spec.n_eep + e, 0)
                    ex[o + 1:o + 1 + n_filt] = True
    return ex


def _first_bad(bad, got, want, what):
    if bad.any():
        k = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} differ; first at {k}: got {got[k]!r}, want {want[k]!r}")


def check_moments(got, want, pivot_dev, exact=None, what="moments"):
    """got / want [n_lines, 5].  pivot_dev [n_lines]: the largest |v - pivot| of the line in the reference (the scale of SUMSQ's
    error).  exact [n_lines] bool: lines whose values are copies, so that N, SUM, SUMSQ, MIN and MAX must all agree bit for bit
    (the caller gives both sides the same pivots): what holds the order of the rows and the unfused square."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    n = want[:, br.N]
    _first_bad(got[:, br.N] != n, got[:, br.N], n, what + ": N")
    has = n > 0
    for c, name in ((br.MIN, "MIN"), (br.MAX, "MAX")):
        _first_bad(~has & (got[:, c] != want[:, c]), got[:, c], want[:, c], f"{what}: {name} of an empty line")
        with np.errstate(invalid="ignore"):              # (an empty line's inf - inf)
            close = np.abs(got[:, c] - want[:, c]) <= MAG_TOL
        _first_bad(has & ~close, got[:, c], want[:, c], f"{what}: {name}")
        if exact is not None:
            _first_bad(exact & has & (got[:, c] != want[:, c]), got[:, c], want[:, c], f"{what}: {name} of a copied column, bit for bit")
    _first_bad(~(np.abs(got[:, br.SUM] - want[:, br.SUM]) <= n * MAG_TOL), got[:, br.SUM], want[:, br.SUM], what + ": SUM")
    tol2 = 2.0 * n * MAG_TOL * pivot_dev + n * MAG_TOL ** 2
    _first_bad(~(np.abs(got[:, br.SUMSQ] - want[:, br.SUMSQ]) <= tol2), got[:, br.SUMSQ], want[:, br.SUMSQ], what + ": SUMSQ")
    if exact is not None:
        for c, name in ((br.SUM, "SUM"), (br.SUMSQ, "SUMSQ")):
            _first_bad(exact & (got[:, c] != want[:, c]), got[:, c], want[:, c], f"{what}: {name} of a copied column, bit for bit")


def pivot_deviation(vals, pivot):
    """max_r |v - pivot| per line (0 for an empty line)"""
    with np.errstate(invalid="ignore"):
        d = np.abs(vals - (0.0 if pivot is None else np.asarray(pivot)[None, :]))
    return np.nan_to_num(np.nanmax(np.where(np.isnan(d), -np.inf, d), axis=0), neginf=0.0)


def assert_edges_clear(vals, edges):
    """On the reference alone: every value lies more than EDGE_MARGIN from every edge of its line."""
    edges = np.asarray(edges, dtype=np.float64).reshape(vals.shape[1], -1)
    with np.errstate(invalid="ignore"):
        d = np.abs(vals[:, :, None] - edges[None, :, :])
    d = np.where(np.isnan(d), np.inf, d)
    assert d.min() > EDGE_MARGIN, f"a reference value lies {d.min():.3g} from an edge"


def check_bins(got, want, vals, edges, what="bins"):
    """Every bin word equal as an integer, after the edges have been shown clear of the reference's values."""
    assert_edges_clear(vals, edges)
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    _first_bad(got != want, got, want, what)


def check_bins_tied(got, want, vals, edges, exact, what="bins with ties"):
    """check_bins where a value may also sit exactly ON an edge of a copied column (exact [n_lines]): the device's value there is
    the reference's, bit for bit, so the word is decided -- closed on the left.  Anywhere else the clearance holds as in check_bins."""
    edges = np.asarray(edges, dtype=np.float64).reshape(vals.shape[1], -1)
    with np.errstate(invalid="ignore"):
        d = np.abs(vals[:, :, None] - edges[None, :, :])
    d = np.where(np.isnan(d), np.inf, d)
    d = np.where((d == 0.0) & np.asarray(exact, dtype=bool)[None, :, None], np.inf, d)
    assert d.min() > EDGE_MARGIN, f"a reference value lies {d.min():.3g} from an edge"
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    _first_bad(got != want, got, want, what)


def check_levels(levels, vals):
    """a N is never within 1e-9 of an integer, for any line's N"""
    counts = np.unique((~np.isnan(vals)).sum(axis=0))
    for a in levels:
        for n in counts[counts > 0]:
            assert abs(a * n - round(a * n)) > 1e-9, (a, n)


def check_brackets(res, vals, levels, what="brackets"):
    """Each final bracket [lo, hi) of hostlib.cmd_band contains the reference's order statistic x_(ceil(a N)); every line with
    values must be final.  Returns the number of brackets checked."""
    check_levels(levels, vals)
    lo, hi, fin = np.asarray(res["lo"]), np.asarray(res["hi"]), np.asarray(res["final"])
    n_lines = vals.shape[1]
    assert lo.shape == (n_lines, len(levels))
    n_checked = 0
    for l in range(n_lines):
        for k, a in enumerate(levels):
            x, _, n = br.order_statistic(vals, l, a)
            if n == 0:                                     # an empty line: the loop must have seen no counted mass (flag 1, kSivNoMass)
                assert np.asarray(res["flags"])[l] & 1, f"{what}: line {l} is empty in the reference, not in the loop"
                continue
            assert fin[l, k], f"{what}: line {l}, level {a}: not final"
            if not (lo[l, k] <= x < hi[l, k]):
                raise AssertionError(f"{what}: line {l}, level {a}: [{lo[l, k]!r}, {hi[l, k]!r}) does not contain x_({math.ceil(a * n)}) = {x!r} of {n}")
            n_checked += 1
    return n_checked
