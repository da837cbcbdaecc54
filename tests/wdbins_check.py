"""The comparator of b9_wd_bins against tests/wdbins_ref.py, the lines' own edges for parity and the checks of the intervals
loop, shared by the CPU tests (tests/test_wdbins_host.py: every mutation of the reference is rejected, the fixtures' conditions
hold) and the GPU tests (tests/test_gpu_wdbins.py)."""
import functools

import numpy as np

import wdbins_ref as br
import wdmoments_check as wc
import wdmoments_ref as wr
from base_amd import abi

RTOL = 1e-9               # per column, plus RTOL of the line's total as the absolute floor
MARGIN = 10.0             # an edge lies at least this many tolerances from every node value of its line
N_EDGES = 31
EPS = 1e-12


def assert_close(got, want, what=""):
    """Every column within rtol = 1e-9, plus 1e-9 of the line's reference total: a column is a sum of weights that add up to
    the total, so that is the scale a rounding error is relative to."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = ~(np.abs(got - want) <= RTOL * want[..., -1:] + RTOL * np.abs(want))
    if bad.any():
        k = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} entries differ; first at {k}: got {got[k]!r}, want {want[k]!r}")


def rejects(check, *args, **kw):
    try:
        check(*args, **kw)
    except AssertionError:
        return True
    return False


def margin_of(e, v, tol):
    """The distance of edge e from the nearest node value, in that node's tolerances."""
    return float(np.min(np.abs(v - e) / tol)) if len(v) else np.inf


def own_edges(lines_by_row, rows, n_wd, mask, n_edges=N_EDGES):
    """(edges [n_wd, n_sel, n_edges], replaced [n_wd, n_sel], margin [n_wd, n_sel]) from the reference alone.  Near each level
    k / (n_edges + 1) of a line's pooled (row x node) weighted CDF: the midpoint of the widest gap -- in units of the
    neighbours' tolerance -- between neighbouring node values within 1/64 of the level.  An edge closer than MARGIN
    tolerances to any node value of its line, or equal to an earlier one, is replaced by one above the line's largest value.
    A line without counted mass gets [0, 1] cut evenly."""
    sel = br.selected(mask)
    edges = np.zeros((n_wd, len(sel), n_edges))
    replaced = np.zeros((n_wd, len(sel)), dtype=int)
    margin = np.full((n_wd, len(sel)), np.inf)
    for c in range(n_wd):
        for s, q in enumerate(sel):
            v, m, tol = br.line_mixture(lines_by_row, rows, c, q)
            if len(v) == 0 or not m.sum() > 0:
                edges[c, s] = np.linspace(0.0, 1.0, n_edges)
                continue
            cw = np.cumsum(m) / m.sum()
            top, out = float(v[-1]), []

            def above():
                replaced[c, s] += 1
                return top + replaced[c, s] * (abs(top) + 1.0)
            for k in range(1, n_edges + 1):
                level = k / (n_edges + 1.0)
                near = np.flatnonzero((cw >= level - 1.0 / 64) & (cw <= level + 1.0 / 64))
                if len(near):
                    lo, hi = max(near[0] - 1, 0), min(near[-1] + 1, len(v) - 1)
                else:
                    i = int(np.searchsorted(cw, level))
                    lo, hi = max(i - 1, 0), min(i, len(v) - 1)
                e = None
                if hi > lo:
                    gap = (v[lo + 1:hi + 1] - v[lo:hi]) / np.maximum(tol[lo + 1:hi + 1], tol[lo:hi])
                    j = lo + int(np.argmax(gap))
                    e = 0.5 * (v[j] + v[j + 1])
                    if e in out or not margin_of(e, v, tol) >= MARGIN:
                        e = None
                out.append(above() if e is None else e)
            edges[c, s] = np.sort(out)
            margin[c, s] = min(margin_of(e, v, tol) for e in edges[c, s])
    assert np.all(np.diff(edges, axis=2) > 0)
    return edges, replaced, margin


def inner_bins_with_mass(acc):
    """per line: the number of inner bins (columns 1 .. B) above 1e-3 of its counted mass, and that mass"""
    acc = np.asarray(acc)
    B = acc.shape[-1] - 3
    C = acc[..., :B + 2].sum(axis=-1)
    return (acc[..., 1:B + 1] > 1e-3 * C[..., None]).sum(axis=-1), C


@functools.lru_cache(maxsize=None)
def parity_lines(key):
    """(lines_by_row, edges [150, 6, 31], replaced, margin) of wdmoments_check.parity_fixture(key): computed once and shared."""
    pack_d, cl, priors, rows, n_pops, n_nodes = wc.parity_fixture(key)[:6]
    lines = [br.row_lines(pack_d, cl, par, n_pops, n_nodes) for par in rows]
    edges, replaced, margin = own_edges(lines, rows, len(wr.wd_stars(cl)), br.ALL)
    for a in (edges, replaced, margin):
        a.setflags(write=False)
    return lines, edges, replaced, margin


def sub_edges(edges, n_bins):
    """n_bins + 1 of a line's 31 own edges, spread over them (all of them for 30 bins)."""
    pick = np.round(np.linspace(0, edges.shape[-1] - 1, n_bins + 3)[1:-1]).astype(int) if n_bins < edges.shape[-1] - 1 else np.arange(edges.shape[-1])
    return np.ascontiguousarray(edges[..., pick])


def reference_rows(lines_by_row, n_wd, mask, edges):
    """x [rows, n_wd, n_sel, B + 3] of the reference, row by row."""
    return np.stack([br.increments_of(lines, n_wd, mask, edges) for lines in lines_by_row])


def summed(x):
    want = np.zeros(x.shape[1:])
    for r in range(x.shape[0]):
        want = want + x[r]
    return want


# ---- the intervals loop against the reference CDF -------------------------------------------------------------------------------
def assert_brackets(lines_by_row, rows, n_wd, mask, levels, lo, hi, final=None, tol=None, label=""):
    """lo, hi, final [n_wd * n_sel, m].  Every bracket of every line with counted mass contains its level of the reference
    CDF of the pooled (row x node) mixture within EPS; a bracket reported final is final: hi - lo <= tol max(|lo|, |hi|), or hi
    the next double after lo, or its mass sits in a single node value.  Returns the lines with counted mass [n_wd * n_sel]."""
    sel = br.selected(mask)
    has = np.zeros(n_wd * len(sel), dtype=bool)
    worst_over = worst_under = -np.inf
    for c in range(n_wd):
        for s, q in enumerate(sel):
            line = c * len(sel) + s
            v, m, _ = br.line_mixture(lines_by_row, rows, c, q)
            if len(v) == 0 or not m.sum() > 0:
                continue
            has[line] = True
            for l, a in enumerate(levels):
                x, y = lo[line, l], hi[line, l]
                assert not np.isnan(x) and not np.isnan(y) and x < y, f"{label}: line ({c}, {q}) with counted mass has no bracket"
                over = (br.cdf(v, m, x) if np.isfinite(x) else (0.0 if x < 0 else 1.0)) - a
                under = a - (br.cdf(v, m, y) if np.isfinite(y) else (1.0 if y > 0 else 0.0))
                worst_over, worst_under = max(worst_over, over), max(worst_under, under)
                assert over <= EPS, f"{label}: line ({c}, {br.NAMES[q]}), level {a}: F(lo) exceeds the level by {over:.3g}"
                assert under <= EPS, f"{label}: line ({c}, {br.NAMES[q]}), level {a}: F(hi) falls short of the level by {under:.3g}"
                if final is not None and final[line, l]:
                    inside = v[(v >= x) & (v < y) & (m > 0)]
                    ok = (y - x <= tol * max(abs(x), abs(y))) or y == np.nextafter(x, np.inf) or len(np.unique(inside)) == 1
                    assert ok, f"{label}: line ({c}, {br.NAMES[q]}), level {a}: [{x!r}, {y!r}) is reported final and is not"
    print(f"{label}: {int(has.sum())} lines with counted mass; largest F(lo) - a = {worst_over:.3g}, largest a - F(hi) = {worst_under:.3g}")
    return has
