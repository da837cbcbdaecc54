"""numpy statement of b9_ratio_hist (tests only): the (primary-mass bin, mass-ratio node) increments of every (row, star), built
on moments_ref.star_nodes (terms, masses, ratios, populations of every finite node), moments_ref.weights,
moments_ref.membership and masshist_ref.bin_index.  Shares no code with the kernels.

For row r and star i: w = exp(t - logsumexp t) over ALL the star's nodes, p the membership; a node of primary mass M1 and
ratio q = j / Q has mass bin b = searchsorted(edges, M1, side="right") - 1 (e_b <= M1 < e_(b+1)) and ratio node
j = rint(q Q);  x[b Q + j] = p sum w over the nodes of that (b, j),  x[n_mbins Q] = p.  A WD-stage star has q = 0 only.  A node
outside the edges falls in no cell but still normalises.  A row outside the grid, and a star with no finite term, contribute
nothing.  star_cells adds the rows in ascending order; row_cells[r] adds the stars in ascending order
(masshist_ref.accumulate / row_sums).

Also the three binaryStats tables restated with np.percentile (binary_table, ratio_dist_table, star_ratio_table)."""
import numpy as np

import masshist_ref as hr
import moments_ref as mr
from base_amd import abi

MUTATIONS = ("transpose_cells", "ratio_from_secondary_bin", "wd_over_all_ratios", "normalise_in_range", "drop_membership")


def increments(pack_d, cl, par, n_pops, K, n_q, mass_edges, nodes=None, transpose_cells=False, ratio_from_secondary_bin=False,
               wd_over_all_ratios=False, normalise_in_range=False, drop_membership=False):
    """x[star, n_mbins Q + 1] of one parameter row.  The keyword flags are the five MUTATIONS the comparators must reject:
    transpose_cells           the cell index j n_mbins + b instead of b Q + j
    ratio_from_secondary_bin  the ratio node not the node's own j but rint(q' Q) of the ratio q' = e / M1 that the lower edge e
                              of the SECONDARY mass's bin gives (the ratio read back from a binned secondary mass)
    wd_over_all_ratios        a WD-stage star's weight spread evenly over all Q ratio nodes of its mass bin
    normalise_in_range        the cells normalised by their own sum instead of by all nodes
    drop_membership           p = 1"""
    edges = np.asarray(mass_edges, dtype=np.float64)
    nb, Q = len(edges) - 1, int(n_q)
    nc = nb * Q
    n = len(cl["mass1"])
    x = np.zeros((n, nc + 1))
    if nodes is None:
        nodes = mr.star_nodes(pack_d, cl, par, n_pops, K, n_q)
    if nodes is None:
        return x
    wd = np.asarray(cl["stage"]) == abi.STAGE_WD
    for i in range(n):
        t, m, q, _ = nodes[i]
        if len(t) == 0:
            continue
        w, L = mr.weights(nodes[i])
        p = 1.0 if drop_membership else mr.membership(cl, i, L)
        b = hr.bin_index(edges, m)
        j = np.rint(q * Q).astype(int)
        if ratio_from_secondary_bin:
            b2 = hr.bin_index(edges, q * m)
            has = (q > 0) & (b2 >= 0) & (b2 < nb)
            j = np.where(has, np.clip(np.rint(edges[np.clip(b2, 0, nb - 1)] / m * Q).astype(int), 0, Q - 1), 0)
        ok = (b >= 0) & (b < nb)
        cell = j * nb + b if transpose_cells else b * Q + j
        h = np.bincount(cell[ok], weights=w[ok], minlength=nc)[:nc]
        if wd_over_all_ratios and wd[i]:
            per_bin = h.reshape((Q, nb)).sum(axis=0) if transpose_cells else h.reshape((nb, Q)).sum(axis=1)
            h = np.repeat(per_bin / Q, Q)
        if normalise_in_range and h.sum() > 0:
            h = h / h.sum()
        x[i, :nc] = p * h
        x[i, nc] = p
    return x


def all_increments(pack_d, cl, rows, n_pops, K, n_q, mass_edges, nodes_by_row=None, **kw):
    """x[row, star, n_mbins Q + 1]"""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
    return np.stack([increments(pack_d, cl, par, n_pops, K, n_q, mass_edges,
                                nodes=None if nodes_by_row is None else nodes_by_row[r], **kw) for r, par in enumerate(rows)])


def reference(pack_d, cl, rows, n_pops, K, n_q, mass_edges, nodes_by_row=None, **kw):
    """(star_cells, row_cells)"""
    x = all_increments(pack_d, cl, rows, n_pops, K, n_q, mass_edges, nodes_by_row, **kw)
    return hr.accumulate(x), hr.row_sums(x)


# ---- the binaryStats tables -------------------------------------------------------------------------------------------------
def _stats(v):
    return [np.mean(v), np.std(v)] + list(np.percentile(v, [16, 50, 84]))


def _lines(row_cells, n_mbins, Q):
    """Per line (the mass bins, then "all"): the cells [rows, Q] of the rows with member > 0 and N > 0."""
    rc = np.asarray(row_cells, dtype=np.float64).reshape(-1, n_mbins * Q + 1)
    cells = rc[:, :n_mbins * Q].reshape(-1, n_mbins, Q)
    member = rc[:, -1] > 0
    for ln in range(n_mbins + 1):
        c = cells[:, ln, :] if ln < n_mbins else cells.sum(axis=1)
        yield ln, c[member & (c.sum(axis=1) > 0)]


def counts(Q, q_min):
    """Which ratio nodes count as a binary at q_min: j >= 1 and j / Q >= q_min."""
    j = np.arange(Q)
    return (j >= 1) & (j / float(Q) >= q_min)


def binary_table(row_cells, mass_edges, Q, q_min=0.0):
    edges = np.asarray(mass_edges, dtype=np.float64)
    nb = len(edges) - 1
    out = np.zeros((nb + 1, 13))
    sel = counts(Q, q_min)
    for ln, c in _lines(row_cells, nb, Q):
        out[ln, 0], out[ln, 1] = (edges[ln], edges[ln + 1]) if ln < nb else (edges[0], edges[-1])
        out[ln, 2] = len(c)
        if len(c):
            N = c.sum(axis=1)
            out[ln, 3:8] = _stats(N)
            out[ln, 8:13] = _stats(c[:, sel].sum(axis=1) / N)
    return out


def ratio_dist_table(row_cells, n_mbins, Q):
    out = np.zeros((n_mbins + 1, Q, 8))
    for ln, c in _lines(row_cells, n_mbins, Q):
        out[ln, :, 0] = np.arange(Q)
        out[ln, :, 1] = np.arange(Q) / float(Q)
        out[ln, :, 2] = len(c)
        if len(c):
            frac = c / c.sum(axis=1, keepdims=True)
            for j in range(Q):
                out[ln, j, 3:8] = _stats(frac[:, j])
    return out


def star_ratio_table(star_cells, n_mbins, Q, n_rows_in_grid, q_min=0.0):
    sc = np.asarray(star_cells, dtype=np.float64).reshape(-1, n_mbins * Q + 1)
    out = np.zeros((len(sc), 4 + Q))
    out[:, 0] = n_rows_in_grid
    if n_rows_in_grid > 0:
        out[:, 1] = sc[:, -1] / n_rows_in_grid
    live = sc[:, -1] > 0
    S = sc[live, :n_mbins * Q].reshape(-1, n_mbins, Q).sum(axis=1)
    tot = sc[live, -1:]
    out[live, 2] = S.sum(axis=1) / tot[:, 0]
    out[live, 3] = S[:, counts(Q, q_min)].sum(axis=1) / tot[:, 0]
    out[live, 4:] = S / tot
    return out
