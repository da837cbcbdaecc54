"""Comparators of b9_mass_hist's outputs against tests/masshist_ref.py, used by the GPU suite and by the CPU suite that
checks the comparators' own power (tests/test_masshist_host.py).

Tolerance: rtol 1e-9 -- the project's per-star tolerance -- and, because the kernels may prune terms
more than 40 e-folds down, atol = N_nodes e^-40 per star entry (N_nodes: the nodes of a star's grid, all populations), times
the number of rows that were added; a row_hist entry sums n_stars of them."""
import numpy as np

RTOL = 1e-9


def star_atol(n_nodes, n_rows=1):
    return n_rows * n_nodes * np.exp(-40.0)


def largest_rel(got, want, floor=1e-6):
    """The largest relative difference among the entries above `floor` (below it the pruning's atol takes over: the reference
    keeps terms of e^-200 that the kernels rightly drop)."""
    got, want = np.asarray(got), np.asarray(want)
    nz = np.abs(want) > floor
    return float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz]))) if nz.any() else 0.0


def assert_star_hist(got, want, n_nodes, n_rows):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=star_atol(n_nodes, n_rows), err_msg="star_hist")


def assert_row_hist(got, want, n_nodes, n_stars):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=n_stars * star_atol(n_nodes), err_msg="row_hist")


def assert_hist(got_star, got_rows, want_star, want_rows, n_nodes, n_stars):
    assert_star_hist(got_star, want_star, n_nodes, len(want_rows))
    assert_row_hist(got_rows, want_rows, n_nodes, n_stars)


# ---- the cases' edges and figures, from the reference alone -----------------------------------------------------------------
def reference_values(nodes_by_row, quantity):
    """(values, weights) of every counting node of every (row, star) of the reference."""
    import masshist_ref as hr
    import moments_ref as mr
    vs, ws = [], []
    for nr in nodes_by_row:
        if nr is None:
            continue
        for nd in nr:
            if len(nd[0]) == 0:
                continue
            w, _ = mr.weights(nd)
            v, c = hr.node_values(nd, quantity)
            vs.append(v[c]); ws.append(w[c])
    if not vs:
        return np.empty(0), np.empty(0)
    return np.concatenate(vs), np.concatenate(ws)


def quantile_edges(nodes_by_row, quantity, n_bins, fallback=(0.02, 16.0)):
    """n_bins + 1 edges that put about the same posterior weight (all stars, all rows) in every bin -- fine where the stars
    are, so that a star's posterior spreads over several bins -- with the two outer edges beyond every node, then separated
    from every node value by 1e-9 relative (masshist_ref.separate_edges).  Without a counting node (SECONDARY at one mass
    ratio): log-spaced over `fallback`."""
    import masshist_ref as hr
    v, w = reference_values(nodes_by_row, quantity)
    if len(v) == 0:
        return fallback[0] * (fallback[1] / fallback[0]) ** (np.arange(n_bins + 1) / n_bins)
    o = np.argsort(v)
    v, w = v[o], w[o]
    cw = np.cumsum(w) / w.sum()
    e = np.concatenate([[v[0] * 0.9], np.interp(np.arange(1, n_bins) / n_bins, cw, v), [v[-1] * 1.1]])
    for i in range(1, len(e)):
        if e[i] <= e[i - 1] * (1 + 1e-6):
            e[i] = e[i - 1] * (1 + 1e-6)
    return hr.separate_edges(e, v)


def non_vacuity(star_hist, n_rows_counted):
    """(live stars, stars with two or more bins above 1e-3 of their total, stars whose mean membership lies strictly inside
    (0.01, 0.99)) of a reference star_hist."""
    sh = np.asarray(star_hist)
    nb = sh.shape[1] - 1
    live = sh[:, nb] > 0
    two = ((sh[:, :nb] > 1e-3 * sh[:, nb:]).sum(axis=1) >= 2) & live
    mem = sh[:, nb] / max(n_rows_counted, 1)
    return int(live.sum()), int(two.sum()), int(((mem > 0.01) & (mem < 0.99)).sum())
