"""numpy statement of b9_phot_resid (tests only): the per-filter residual increments of every (row, star), built on
moments_ref.star_nodes (terms, masses, ratios, populations of every finite node), moments_ref.weights and
moments_ref.membership, with the node magnitudes from synth.forward_mags at each node's (M1, q, pop, wd_type).  Shares no
code with the kernels.

For row r and star i: w = exp(t - logsumexp t) over the star's nodes, p the membership; pred_f the node's combined apparent
magnitude; the pivot c_f = obs_f where sigma_f > 0, else 0; d_f = pred_f - c_f;
    x = (1, p, p sum w d_0, p sum w d_0^2, ..., p sum w d_(nf-1), p sum w d_(nf-1)^2).
A row outside the grid, and a star with no finite term, contribute nothing.  star_resid adds the rows in ascending order;
row_resid[r] = (sum_i p_i, then per filter over the stars with sigma > 0:  N = sum p, R = -sum x[2+2f] / sigma,
C = sum x[3+2f] / sigma^2, W = sum p / sigma^2, D = -sum x[2+2f] / sigma^2), the stars in ascending order.

Also the two derived tables (star_table, filter_table) restated with numpy, and six MUTATIONS (keyword flags) that the
comparators of tests/resid_check.py must reject."""
import numpy as np

import moments_ref as mr
from base_amd import abi, synth

STAR_MUTATIONS = ("no_pivot", "second_from_d", "drop_pop_weight", "drop_membership")
ROW_MUTATIONS = ("count_unused", "flip_z")


def ncol(nf):
    return 2 + 2 * nf


def pivots(cl):
    """c[star, filter]: the observation where the filter is used, else 0."""
    obs, sig = np.asarray(cl["obs"], dtype=np.float64), np.asarray(cl["sigma"], dtype=np.float64)
    return np.where(sig > 0, obs, 0.0)


def node_mags(pack_d, cl, par, nodes, cache=None):
    """Per star the magnitudes [nodes, nf] of its nodes (None without nodes)."""
    cache = {} if cache is None else cache
    wd_stage = np.asarray(cl["stage"]) == abi.STAGE_WD
    out = []
    for i, (t, m, q, k) in enumerate(nodes):
        if len(t) == 0:
            out.append(None)
            continue
        ty = int(np.asarray(cl["wd_type"])[i]) if wd_stage[i] else 0        # (MS/RGB nodes lie below the tip: the type is not read)
        mags = np.empty((len(t), pack_d["n_filt"]))
        for pop in np.unique(k):
            sel = k == pop
            key = (int(pop), ty, m[sel].tobytes(), q[sel].tobytes())
            if key not in cache:
                cache[key] = synth.forward_mags(pack_d, par, m[sel], q[sel], np.full(int(sel.sum()), ty, int), pop=int(pop))
            mags[sel] = cache[key]
        out.append(mags)
    return out


def increments(pack_d, cl, par, n_pops, K, n_q, nodes=None, no_pivot=False, second_from_d=False, drop_pop_weight=False,
               drop_membership=False):
    """(x[star, 2 + 2 nf], bound[star, 2 + 2 nf], absx[star, 2 + 2 nf]) of one parameter row.  bound: what one dropped unit of
    weight can move an entry by (1 for MEMBER, max |d_f| and max d_f^2 over the star's nodes for the sums, 0 for ROWS);
    absx: p sum w |d_f| in the first-moment columns (the scale of their rounding), |x| elsewhere.  The keyword flags are four
    of the MUTATIONS."""
    nf = pack_d["n_filt"]
    n = len(cl["mass1"])
    x, bound, absx = np.zeros((n, ncol(nf))), np.zeros((n, ncol(nf))), np.zeros((n, ncol(nf)))
    if drop_pop_weight and n_pops == 2:
        par = np.array(par, dtype=np.float64)
        par[abi.P_LAMBDA] = 0.5
        nodes = None
    if nodes is None:
        nodes = mr.star_nodes(pack_d, cl, par, n_pops, K, n_q)
    if nodes is None:
        return x, bound, absx
    c = np.zeros((n, nf)) if no_pivot else pivots(cl)
    mags = node_mags(pack_d, cl, par, nodes)
    for i in range(n):
        if mags[i] is None:
            continue
        w, L = mr.weights(nodes[i])
        p = 1.0 if drop_membership else mr.membership(cl, i, L)
        d = mags[i] - c[i][None, :]
        x[i, 0], x[i, 1] = 1.0, p
        x[i, 2::2] = p * (w[:, None] * d).sum(axis=0)
        x[i, 3::2] = p * (w[:, None] * (d if second_from_d else d * d)).sum(axis=0)
        bound[i, 1] = 1.0
        bound[i, 2::2] = np.abs(d).max(axis=0)
        bound[i, 3::2] = (d * d).max(axis=0)
        absx[i] = np.abs(x[i])
        absx[i, 2::2] = p * (w[:, None] * np.abs(d)).sum(axis=0)
    return x, bound, absx


def nodes_of_rows(pack_d, cl, rows, n_pops, K, n_q):
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
    return [mr.star_nodes(pack_d, cl, par, n_pops, K, n_q) for par in rows]


def all_increments(pack_d, cl, rows, n_pops, K, n_q, nodes_by_row=None, **kw):
    """(x, bound, absx), each [row, star, 2 + 2 nf]"""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
    parts = [increments(pack_d, cl, par, n_pops, K, n_q, nodes=None if nodes_by_row is None else nodes_by_row[r], **kw)
             for r, par in enumerate(rows)]
    return tuple(np.stack([p[k] for p in parts]) for k in range(3))


def accumulate(x, start=None):
    """star_resid: the rows' increments added in ascending row order."""
    acc = np.zeros(x.shape[1:]) if start is None else np.array(start, dtype=np.float64)
    for xr in x:
        acc = acc + xr
    return acc


def row_sums(x, cl, count_unused=False, flip_z=False):
    """row_resid [row, 1 + 5 nf]: the stars added in ascending order.  count_unused / flip_z: two of the MUTATIONS (an unused
    filter counted with sigma = 1; z taken as computed minus observed)."""
    sig = np.asarray(cl["sigma"], dtype=np.float64)
    n_rows, n, nc = x.shape
    nf = (nc - 2) // 2
    sgn = 1.0 if flip_z else -1.0
    out = np.zeros((n_rows, 1 + 5 * nf))
    for r in range(n_rows):
        a = np.zeros(1 + 5 * nf)
        for i in range(n):
            p = x[r, i, 1]
            a[0] = a[0] + p
            for f in range(nf):
                s = sig[i, f]
                if not s > 0:
                    if not count_unused:
                        continue
                    s = 1.0
                a[1 + 5 * f] = a[1 + 5 * f] + p
                a[2 + 5 * f] = a[2 + 5 * f] + sgn * x[r, i, 2 + 2 * f] / s
                a[3 + 5 * f] = a[3 + 5 * f] + x[r, i, 3 + 2 * f] / s ** 2
                a[4 + 5 * f] = a[4 + 5 * f] + p / s ** 2
                a[5 + 5 * f] = a[5 + 5 * f] + sgn * x[r, i, 2 + 2 * f] / s ** 2
        out[r] = a
    return out


def reference(pack_d, cl, rows, n_pops, K, n_q, nodes_by_row=None, **mutation):
    """(star_resid, row_resid, x, bound, absx) of the rows."""
    star_kw = {k: v for k, v in mutation.items() if k in STAR_MUTATIONS}
    row_kw = {k: v for k, v in mutation.items() if k in ROW_MUTATIONS}
    x, bound, absx = all_increments(pack_d, cl, rows, n_pops, K, n_q, nodes_by_row, **star_kw)
    return accumulate(x), row_sums(x, cl, **row_kw), x, bound, absx


# ---- the derived tables -----------------------------------------------------------------------------------------------------
def star_moments_of(acc, cl):
    """(mean d [star, nf], second moment [star, nf], variance [star, nf]) of an accumulator; zeros without membership weight."""
    acc = np.asarray(acc, dtype=np.float64)
    m = acc[:, 1] > 0
    m1, m2 = np.zeros_like(acc[:, 2::2]), np.zeros_like(acc[:, 3::2])
    m1[m], m2[m] = acc[m, 2::2] / acc[m, 1:2], acc[m, 3::2] / acc[m, 1:2]
    return m1, m2, m2 - m1 ** 2


def star_table(acc, cl, no_pivot=False):
    """[star, 2 + 4 nf]: rows, member, then per filter predMag, predSd, resid, rmsZ, stated independently of b9h_resid_table.
    no_pivot: the table of an accumulator that was formed WITHOUT the pivot (the mutation's own reading)."""
    acc = np.asarray(acc, dtype=np.float64)
    obs, sig = np.asarray(cl["obs"], dtype=np.float64), np.asarray(cl["sigma"], dtype=np.float64)
    n, nf = obs.shape
    used = sig > 0
    c = np.where(used, obs, 0.0)
    out = np.zeros((n, 2 + 4 * nf))
    out[:, 0] = acc[:, 0]
    live = acc[:, 0] > 0
    out[live, 1] = acc[live, 1] / acc[live, 0]
    m1, m2, var = star_moments_of(acc, cl)
    mem = (acc[:, 1] > 0)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        pred = np.where(mem, (0.0 if no_pivot else c) + m1, 0.0)
        out[:, 2::4] = pred
        out[:, 3::4] = np.where(mem, np.sqrt(np.maximum(0.0, var)), 0.0)
        out[:, 4::4] = np.where(mem & used, obs - pred, 0.0)
        out[:, 5::4] = np.where(mem & used, np.sqrt(np.maximum(m2, 0.0)) / np.where(used, sig, 1.0), 0.0)
    return out


FILTER_COLUMNS = ("nRows",) + tuple(q + "_" + s for q in ("meanZ", "chi2", "offset") for s in ("mean", "sd", "p16", "p50", "p84"))


def filter_table(row_resid, nf):
    """[nf, 16] (FILTER_COLUMNS): over the rows with N_f > 0 the mean, population sd and 16th / 50th / 84th percentiles
    (np.percentile's default) of R_f / N_f, C_f / N_f and D_f / W_f."""
    rr = np.asarray(row_resid, dtype=np.float64).reshape(-1, 1 + 5 * nf)
    out = np.zeros((nf, 16))
    for f in range(nf):
        N, R, Cc, W, D = (rr[:, 1 + 5 * f + k] for k in range(5))
        use = N > 0
        out[f, 0] = use.sum()
        if not use.any():
            continue
        with np.errstate(invalid="ignore", divide="ignore"):
            qs = (R[use] / N[use], Cc[use] / N[use], np.where(W[use] > 0, D[use] / np.where(W[use] > 0, W[use], 1.0), 0.0))
        for k, v in enumerate(qs):
            out[f, 1 + 5 * k] = v.mean()
            out[f, 2 + 5 * k] = v.std()
            out[f, 3 + 5 * k:6 + 5 * k] = np.percentile(v, [16, 50, 84])
    return out
