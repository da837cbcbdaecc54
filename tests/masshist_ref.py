"""numpy statement of b9_mass_hist (tests only): the binned increments of every (row, star), built on
moments_ref.star_nodes (terms, masses, ratios, populations of every finite node), moments_ref.weights and
moments_ref.membership.  Shares no code with the kernels.

For row r and star i: w = exp(t - logsumexp t) over ALL the star's nodes, p the membership; the node's value v is M1
(PRIMARY), q M1 for the nodes with q > 0 (SECONDARY) or M1 + q M1 (SYSTEM); bin b = searchsorted(edges, v, side="right") - 1
holds e_b <= v < e_(b+1);  x[b] = p sum_{v in b} w,  x[n_bins] = p.  A row outside the grid, and a star with no finite term,
contribute nothing.  star_hist adds the rows in ascending order; row_hist[r] adds the stars in ascending order.

Also the massFunction table restated with np.percentile (table)."""
import numpy as np

import moments_ref as mr
from base_amd import abi

PRIMARY, SECONDARY, SYSTEM = 0, 1, 2


def node_values(nodes_i, quantity, secondary_on_q=False):
    """(v, counts) of one star's nodes: the value and whether the node takes part in the bins.  secondary_on_q: the MUTATION
    that bins SECONDARY on q instead of q M1."""
    _, m, q, _ = nodes_i
    if quantity == PRIMARY:
        return m, np.ones(len(m), bool)
    m2 = q * m
    if quantity == SECONDARY:
        return (q if secondary_on_q else m2), q > 0
    if quantity == SYSTEM:
        return m + m2, np.ones(len(m), bool)
    raise ValueError("quantity")


def bin_index(edges, v, right_closed=False):
    """Bin of every value: e_b <= v < e_(b+1); -1 or n_bins: in none.  right_closed: the MUTATION e_b < v <= e_(b+1)."""
    return np.searchsorted(edges, v, side="left" if right_closed else "right") - 1


def increments(pack_d, cl, par, n_pops, K, n_q, quantity, edges, nodes=None, right_closed=False, drop_membership=False,
               secondary_on_q=False, drop_pop_weight=False, normalise_in_range=False):
    """x[star, n_bins + 1] of one parameter row.  The keyword flags are the five MUTATIONS the comparators must reject."""
    edges = np.asarray(edges, dtype=np.float64)
    nb = len(edges) - 1
    n = len(cl["mass1"])
    x = np.zeros((n, nb + 1))
    if drop_pop_weight and n_pops == 2:
        par = np.array(par, dtype=np.float64)
        par[abi.P_LAMBDA] = 0.5
        nodes = None
    if nodes is None:
        nodes = mr.star_nodes(pack_d, cl, par, n_pops, K, n_q)
    if nodes is None:
        return x
    for i in range(n):
        if len(nodes[i][0]) == 0:
            continue
        w, L = mr.weights(nodes[i])
        p = 1.0 if drop_membership else mr.membership(cl, i, L)
        v, counts = node_values(nodes[i], quantity, secondary_on_q)
        b = bin_index(edges, v, right_closed)
        ok = counts & (b >= 0) & (b < nb)
        h = np.bincount(b[ok], weights=w[ok], minlength=nb)[:nb]
        if normalise_in_range and h.sum() > 0:
            h = h / h.sum()
        x[i, :nb] = p * h
        x[i, nb] = p
    return x


def all_increments(pack_d, cl, rows, n_pops, K, n_q, quantity, edges, nodes_by_row=None, **kw):
    """x[row, star, n_bins + 1]"""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
    return np.stack([increments(pack_d, cl, par, n_pops, K, n_q, quantity, edges,
                                nodes=None if nodes_by_row is None else nodes_by_row[r], **kw) for r, par in enumerate(rows)])


def accumulate(x, start=None):
    """star_hist: the rows' increments added in ascending row order."""
    acc = np.zeros(x.shape[1:]) if start is None else np.array(start, dtype=np.float64)
    for xr in x:
        acc = acc + xr
    return acc


def row_sums(x):
    """row_hist: the stars' increments of every row added in ascending star order."""
    out = np.zeros((x.shape[0], x.shape[2]))
    for r in range(x.shape[0]):
        a = np.zeros(x.shape[2])
        for i in range(x.shape[1]):
            a = a + x[r, i]
        out[r] = a
    return out


def nodes_of_rows(pack_d, cl, rows, n_pops, K, n_q):
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
    return [mr.star_nodes(pack_d, cl, par, n_pops, K, n_q) for par in rows]


TABLE_COLUMNS = ("lo", "hi", "mean", "sd", "p16", "p50", "p84", "dNdlogM")


def table(row_hist, edges):
    """The massFunction table [n_bins, 8] (TABLE_COLUMNS): over the rows whose member column is > 0, per bin the mean, the
    population standard deviation and the 16th / 50th / 84th percentiles (np.percentile's default, linear interpolation
    between order statistics) of the expected count, and mean / log10(hi / lo) (0 where lo <= 0).  No such row: zeros."""
    edges = np.asarray(edges, dtype=np.float64)
    nb = len(edges) - 1
    rh = np.asarray(row_hist, dtype=np.float64).reshape(-1, nb + 1)
    use = rh[rh[:, nb] > 0]
    out = np.zeros((nb, 8))
    out[:, 0], out[:, 1] = edges[:-1], edges[1:]
    if len(use) == 0:
        return out
    c = use[:, :nb]
    out[:, 2] = c.mean(axis=0)
    out[:, 3] = c.std(axis=0)
    out[:, 4:7] = np.percentile(c, [16, 50, 84], axis=0).T
    for b in range(nb):
        if edges[b] > 0:
            out[b, 7] = out[b, 2] / np.log10(edges[b + 1] / edges[b])
    return out


def separate_edges(edges, values, rel=1e-9):
    """Edges nudged until no value lies within `rel` relative of one (the device forms M1 with an fma, numpy with two
    roundings: a node that close to an edge could fall either way).  values: every reference node value of the case."""
    edges = np.array(edges, dtype=np.float64)
    values = np.sort(np.asarray(values, dtype=np.float64))
    for b in range(len(edges)):
        for _ in range(100):
            k = np.searchsorted(values, edges[b])
            near = [values[j] for j in (k - 1, k) if 0 <= j < len(values)]
            if all(abs(v - edges[b]) > 4 * rel * max(abs(v), abs(edges[b])) for v in near):
                break
            edges[b] *= 1.0 + 16 * rel
        else:
            raise AssertionError("could not separate an edge from the nodes")
    assert np.all(np.diff(edges) > 0)
    return edges
