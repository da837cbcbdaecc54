"""numpy statement of b9_star_bins and of the per-star refinement (tests only), built on moments_ref (terms, weights,
membership) and masshist_ref.node_values.  Shares no code with the kernels or with b9h::refine_star_edges.

For row r and star i with its OWN edges e_i0 < .. < e_iB: w = exp(t - logsumexp t) over ALL the star's nodes, p the membership,
v the node's value; column c = searchsorted(e_i, v, side="right") is 0 below e_i0, 1 + b in bin b (closed on the left) and
B + 1 at or above e_iB;  x[c] = p sum_{v in c} w over the counting nodes,  x[B + 2] = p.  A row outside the grid and a star
with no finite term contribute nothing.  acc adds the rows in ascending order.

The refinement: the levels are taken on the counted mass C = sum of the B + 2 columns; a level's bracket is the column in
which the cumulative sum first reaches a C.  cdf(): F(x) = the mass of v < x over the counted mass, from the nodes directly."""
import numpy as np

import masshist_ref as hr
import moments_ref as mr
from base_amd import abi


def increments(pack_d, cl, par, n_pops, K, n_q, quantity, edges, nodes=None, right_closed=False, drop_membership=False,
               fold_below=False, normalise_in_range=False, neighbour_edges=None):
    """x[star, B + 3] of one parameter row; edges [star, B + 1].  The keyword flags are MUTATIONS the comparators must reject:
    bins closed on the right; membership dropped; `below` folded into bin 0; weights normalised over the edge range instead of
    all nodes; neighbour_edges = i: star i + 1 binned on star i's edges."""
    edges = np.asarray(edges, dtype=np.float64)
    n, B = edges.shape[0], edges.shape[1] - 1
    x = np.zeros((n, B + 3))
    if nodes is None:
        nodes = mr.star_nodes(pack_d, cl, par, n_pops, K, n_q)
    if nodes is None:
        return x
    for i in range(n):
        if len(nodes[i][0]) == 0:
            continue
        w, L = mr.weights(nodes[i])
        p = 1.0 if drop_membership else mr.membership(cl, i, L)
        v, counts = hr.node_values(nodes[i], quantity)
        e = edges[i - 1] if (neighbour_edges is not None and i == neighbour_edges + 1) else edges[i]
        c = np.searchsorted(e, v, side="left" if right_closed else "right")
        h = np.bincount(c[counts], weights=w[counts], minlength=B + 2)
        if fold_below:
            h[1] += h[0]
            h[0] = 0.0
        if normalise_in_range and h[1:B + 1].sum() > 0:
            h[1:B + 1] = h[1:B + 1] / h[1:B + 1].sum()
        x[i, :B + 2] = p * h
        x[i, B + 2] = p
    return x


def accumulate(pack_d, cl, rows, n_pops, K, n_q, quantity, edges, nodes_by_row=None, start=None, **kw):
    """acc[star, B + 3]: the rows' increments added in ascending row order."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
    edges = np.asarray(edges, dtype=np.float64)
    acc = np.zeros((edges.shape[0], edges.shape[1] + 2)) if start is None else np.array(start, dtype=np.float64)
    for r, par in enumerate(rows):
        acc = acc + increments(pack_d, cl, par, n_pops, K, n_q, quantity, edges, nodes=None if nodes_by_row is None else nodes_by_row[r], **kw)
    return acc


def star_mixture(cl, nodes_by_row, i, quantity):
    """(v, m) of star i: the value and the membership-weighted mass p w of every counting node of every row, sorted by value."""
    vs, ms = [], []
    for nr in nodes_by_row:
        if nr is None or len(nr[i][0]) == 0:
            continue
        w, L = mr.weights(nr[i])
        v, counts = hr.node_values(nr[i], quantity)
        vs.append(v[counts]); ms.append(mr.membership(cl, i, L) * w[counts])
    if not vs:
        return np.empty(0), np.empty(0)
    v, m = np.concatenate(vs), np.concatenate(ms)
    o = np.argsort(v, kind="stable")
    return v[o], m[o]


def cdf(v, m, x):
    """F(x): the mass of v < x over the counted mass (v sorted)."""
    return float(m[:np.searchsorted(v, x, side="left")].sum() / m.sum())


SLACK = 1e-13          # "reaches a C" is meant within this much of C, the rounding of the sums: a tie goes to the lower node


def brackets(edges, acc, levels, on_total=False):
    """(lo, hi, C) [n, m], [n, m], [n] of one pass: the column in which the cumulative sum first reaches a C.  on_total: the
    MUTATION that takes the levels on the total column instead of the counted mass."""
    edges, acc = np.asarray(edges, dtype=np.float64), np.asarray(acc, dtype=np.float64)
    n, B = edges.shape[0], edges.shape[1] - 1
    lo, hi = np.full((n, len(levels)), np.nan), np.full((n, len(levels)), np.nan)
    cum = np.cumsum(acc[:, :B + 2], axis=1)
    C = acc[:, B + 2].copy() if on_total else cum[:, B + 1].copy()
    ext = np.concatenate([np.full((n, 1), -np.inf), edges, np.full((n, 1), np.inf)], axis=1)
    for i in range(n):
        if not C[i] > 0:
            continue
        for l, a in enumerate(levels):
            k = min(int(np.searchsorted(cum[i], a * C[i] - SLACK * C[i], side="left")), B + 1)
            lo[i, l], hi[i, l] = ext[i, k], ext[i, k + 1]
    return lo, hi, C


class NumpyEngine:
    """The numpy reference in the place of the device: what hostlib.star_intervals needs of an engine."""

    def __init__(self, pack_d, cl, n_pops, K, n_q, nodes_by_row, max_mass):
        self.pack_d, self.cl, self.n_pops, self.K, self.n_q, self.nodes = pack_d, cl, n_pops, K, n_q, nodes_by_row
        self.n_stars, self.max_mass = len(cl["mass1"]), float(max_mass)
        self.calls = 0

    def star_bins(self, rows, edges, quantity=hr.PRIMARY, acc=None):
        self.calls += 1
        return accumulate(self.pack_d, self.cl, rows, self.n_pops, self.K, self.n_q, quantity, edges, nodes_by_row=self.nodes, start=acc)
