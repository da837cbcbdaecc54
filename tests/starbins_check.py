"""Comparators of b9_star_bins' accumulators and of star_intervals' brackets against tests/starbins_ref.py, and the cases'
per-star edges (from the reference alone).  Used by the GPU suite and by the CPU suite that checks the comparators' own power
(tests/test_starbins_host.py).

Tolerance of an accumulator entry: masshist_check.assert_star_hist's, for every column -- `below` and `above` are bins like the
others.  A bracket [lo, hi) of level a must satisfy F(lo) <= a + EPS and F(hi) >= a - EPS for the reference CDF F of the full
(row x node) membership-weighted mixture, EPS = 1e-12 being the rounding of the sums."""
import numpy as np

import masshist_check as hc
import masshist_ref as hr
import starbins_ref as sr

EPS = 1e-12


def largest_diff(got, want):
    """(largest absolute difference, its index, largest relative difference among the entries above 1e-6)"""
    got, want = np.asarray(got), np.asarray(want)
    d = np.abs(got - want)
    k = np.unravel_index(int(np.argmax(d)), d.shape)
    return float(d[k]), tuple(int(x) for x in k), hc.largest_rel(got, want)


def assert_star_bins(got, want, n_nodes, n_rows, label=""):
    d, k, rel = largest_diff(got, want)
    print(f"{label}: largest difference {d:.3g} at (star, column) {k}; largest relative difference among the entries above 1e-6: {rel:.3g}")
    hc.assert_star_hist(got, want, n_nodes, n_rows)


def own_edges(cl, nodes_by_row, quantity, n_bins, tails=(0.05, 0.95)):
    """edges [n_stars, n_bins + 1]: every star's own weighted quantiles of its node values -- the outer edges at `tails`, so that
    `below` and `above` hold mass, the inner ones evenly in weight between them --, made strictly ascending and separated from
    every node value of that star by 1e-9 relative (masshist_ref.separate_edges).  A star without a counting node: 0.1 .. 8."""
    n = len(cl["mass1"])
    out = np.zeros((n, n_bins + 1))
    for i in range(n):
        v, m = sr.star_mixture(cl, nodes_by_row, i, quantity)
        if len(v) == 0 or not m.sum() > 0:
            out[i] = np.linspace(0.1, 8.0, n_bins + 1)
            continue
        cw = np.cumsum(m) / m.sum()
        e = np.interp(np.linspace(tails[0], tails[1], n_bins + 1), cw, v)
        for b in range(1, len(e)):
            if e[b] <= e[b - 1] * (1 + 1e-6):
                e[b] = e[b - 1] * (1 + 1e-6)
        out[i] = hr.separate_edges(e, v)
    return out


def bins_with_mass(acc):
    """per star: the number of its own bins (columns 1 .. B) above 1e-3 of its counted mass, and that mass"""
    acc = np.asarray(acc)
    B = acc.shape[1] - 3
    C = acc[:, :B + 2].sum(axis=1)
    return (acc[:, 1:B + 1] > 1e-3 * C[:, None]).sum(axis=1), C


def bracket_violations(cl, nodes_by_row, quantity, levels, lo, hi):
    """(F(lo) - a, a - F(hi)) [n, m] against the reference CDF; NaN for a star without counted mass."""
    n, m = lo.shape
    over, under = np.full((n, m), np.nan), np.full((n, m), np.nan)
    for i in range(n):
        v, w = sr.star_mixture(cl, nodes_by_row, i, quantity)
        if len(v) == 0 or not w.sum() > 0:
            continue
        for l, a in enumerate(levels):
            over[i, l] = (sr.cdf(v, w, lo[i, l]) if np.isfinite(lo[i, l]) else (0.0 if lo[i, l] < 0 else 1.0)) - a
            under[i, l] = a - (sr.cdf(v, w, hi[i, l]) if np.isfinite(hi[i, l]) else (1.0 if hi[i, l] > 0 else 0.0))
    return over, under


def assert_brackets(cl, nodes_by_row, quantity, levels, lo, hi, final=None, tol=None, label=""):
    """Every bracket of every star with counted mass contains its level; a bracket reported final is final: hi - lo <= tol
    max(|lo|, |hi|), or hi the next double after lo, or its mass sits in a single node value.  Returns the stars with mass."""
    over, under = bracket_violations(cl, nodes_by_row, quantity, levels, lo, hi)
    has = ~np.isnan(over[:, 0])
    assert not np.isnan(lo[has]).any() and not np.isnan(hi[has]).any(), "a star with counted mass has no bracket"
    print(f"{label}: {int(has.sum())} stars with counted mass; largest F(lo) - a = {np.nanmax(over):.3g}, largest a - F(hi) = {np.nanmax(under):.3g}")
    assert np.all(over[has] <= EPS), f"F(lo) exceeds the level by {np.nanmax(over):.3g}"
    assert np.all(under[has] <= EPS), f"F(hi) falls short of the level by {np.nanmax(under):.3g}"
    assert np.all(lo[has] < hi[has])
    if final is not None:
        for i in np.flatnonzero(has):
            v, w = sr.star_mixture(cl, nodes_by_row, i, quantity)
            for l in range(len(levels)):
                if not final[i, l]:
                    continue
                a, b = lo[i, l], hi[i, l]
                inside = v[(v >= a) & (v < b) & (w > 0)]
                ok = (b - a <= tol * max(abs(a), abs(b))) or b == np.nextafter(a, np.inf) or len(np.unique(inside)) == 1
                assert ok, f"star {i}, level {levels[l]}: [{a!r}, {b!r}) is reported final and is not"
    return has
