"""numpy statement of b9_wd_bins (tests only): the increments [n_wd, n_sel, B + 3] of one parameter row on every line's own
edges, built on wdmoments_ref.star_nodes -- the terms, masses, cooled flags and derived values of every finite node of
b9_sample_wd_mass's grid --, scipy's logsumexp and moments_ref.membership.  Shares no code with the kernels or the C oracle.

A line is (WD-stage star i, s-th selected quantity of the mask, ascending).  A node's value is its ZAMS mass under quantity 0 and
its derived value (wd_mass, prec, log_cool, log_teff, logg) under 1 .. 5, where only COOLED nodes count.  With w = exp(t - L)
and p the membership: column 0 = p sum_{v < e_0} w, column 1 + b = p sum_{e_b <= v < e_(b+1)} w, column B + 1 = p sum_{v >= e_B} w
over the counting nodes, column B + 2 = p.  A row outside the grid and a star with no finite term contribute nothing.

The keyword MUTATIONS are wrong on purpose: the comparator of tests/wdbins_check.py must reject each of them."""
import numpy as np
from scipy.special import logsumexp

import moments_ref
import wdmoments_ref as wr
from base_amd import abi

N_Q = 6
NAMES = ("zamsMass", "wdMass", "precLogAge", "logCoolAge", "logTeff", "logg")
ALL = (1 << N_Q) - 1
MUTATIONS = ("closed_right", "derived_over_all_nodes", "drop_total_uncooled", "drop_pop_weight", "other_line_edges")


def selected(mask):
    return [q for q in range(N_Q) if mask >> q & 1]


def row_lines(pack_d, cl, par, n_pops, n_nodes, drop_pop_weight=False, nodes=None):
    """Per WD-stage star of one row: (p, w, m, cooled, der [node, 5]) over its finite nodes, or None for a star without a
    finite term; None altogether for a row outside the grid."""
    if nodes is None:                                    # (nodes: the row's wdmoments_ref.star_nodes, where the caller has them)
        nodes = wr.star_nodes(pack_d, cl, par, n_pops, n_nodes, drop_pop_weight=drop_pop_weight)
    if nodes is None:
        return None
    out = []
    for c, i in enumerate(wr.wd_stars(cl)):
        t, m, k, cooled, der = nodes[c]
        if len(t) == 0:
            out.append(None)
            continue
        L = logsumexp(t)
        out.append((moments_ref.membership(cl, i, L), np.exp(t - L), m, cooled, der))
    return out


def line_values(line, q, derived_over_all_nodes=False):
    """(v, counts) of a star's nodes under quantity q."""
    p, w, m, cooled, der = line
    if q == 0:
        return m, np.ones(len(m), dtype=bool)
    return der[:, q - 1], (np.ones(len(m), dtype=bool) if derived_over_all_nodes else cooled)


def increments_of(lines, n_wd, mask, edges, closed_right=False, derived_over_all_nodes=False, drop_total_uncooled=False,
                  other_line_edges=False):
    """x [n_wd, n_sel, B + 3] of one row's row_lines on the edges [n_wd, n_sel, B + 1]."""
    sel = selected(mask)
    edges = np.asarray(edges, dtype=np.float64).reshape(n_wd * len(sel), -1)
    B = edges.shape[1] - 1
    if other_line_edges:
        edges = np.roll(edges, 1, axis=0)
    x = np.zeros((n_wd, len(sel), B + 3))
    if lines is None:
        return x
    for c, line in enumerate(lines):
        if line is None:
            continue
        p, w, m, cooled, der = line
        for s, q in enumerate(sel):
            v, cnt = line_values(line, q, derived_over_all_nodes)
            # the number of edges <= v (closed on the left) is the column: 0 below e_0, 1 + b in bin b, B + 1 at or above e_B
            col = np.searchsorted(edges[c * len(sel) + s], v, side="left" if closed_right else "right")
            x[c, s, :B + 2] = p * np.bincount(col[cnt], weights=w[cnt], minlength=B + 2)
            x[c, s, B + 2] = p
            if drop_total_uncooled and q > 0 and not cooled.any():
                x[c, s, B + 2] = 0.0
    return x


def increments(pack_d, cl, par, n_pops, n_nodes, mask, edges, drop_pop_weight=False, **mutation):
    lines = row_lines(pack_d, cl, par, n_pops, n_nodes, drop_pop_weight=drop_pop_weight)
    return increments_of(lines, len(wr.wd_stars(cl)), mask, edges, **mutation)


def accumulate(pack_d, cl, rows, n_pops, n_nodes, mask, edges, acc=None, **mutation):
    """acc [n_wd, n_sel, B + 3]: the rows' increments added in ascending row order (to `acc`, or to zeros)."""
    for par in np.asarray(rows, dtype=np.float64).reshape(-1, abi.B9_NPARAM):
        x = increments(pack_d, cl, par, n_pops, n_nodes, mask, edges, **mutation)
        acc = x if acc is None else np.asarray(acc, dtype=np.float64).reshape(x.shape) + x
    return acc


def node_tol(q, v, der, par):
    """How far the device's value of a node may lie from the reference's: test_gpu_wdmass.check_derived's tolerance of the
    quantity (rtol 1e-9 for the two masses; rtol 1e-9 + atol 1e-9 for the others), times the amplification t / (t - 10^prec)
    of an error in prec where the value follows from the cooling age (log_cool, log_teff, logg)."""
    v = np.asarray(v, dtype=np.float64)
    if q <= 1:
        return 1e-9 * np.abs(v)
    tol = 1e-9 * np.abs(v) + 1e-9
    if q == 2:
        return tol
    t, p = 10.0 ** par[abi.P_LOGAGE], 10.0 ** der[:, 1]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        amp = np.where(t > p, t / np.maximum(t - p, 1e-300), 1.0)
    return tol * np.maximum(amp, 1.0)


def line_mixture(lines_by_row, rows, c, q):
    """(v, mass p w, tol) of line (c, q): every counting node of every row, sorted by value."""
    vs, ms, ts = [], [], []
    for lines, par in zip(lines_by_row, rows):
        if lines is None or lines[c] is None:
            continue
        v, cnt = line_values(lines[c], q)
        p, w, m, cooled, der = lines[c]
        vs.append(v[cnt]); ms.append(p * w[cnt]); ts.append(node_tol(q, v, der, par)[cnt])
    if not vs:
        return np.empty(0), np.empty(0), np.empty(0)
    v, m, t = np.concatenate(vs), np.concatenate(ms), np.concatenate(ts)
    o = np.argsort(v, kind="stable")
    return v[o], m[o], t[o]


def cdf(v, m, x):
    """F(x): the mass of v < x over the counted mass (v sorted)."""
    return float(m[:np.searchsorted(v, x, side="left")].sum() / m.sum())
