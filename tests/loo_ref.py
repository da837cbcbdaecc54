"""numpy statement of b9_filter_loo (tests only): the leave-one-filter-out increments of every (row, star), built on
moments_ref.star_nodes (terms, masses, ratios, populations of every finite node), moments_ref.weights, moments_ref.membership
and resid_ref.node_mags (the node magnitudes).  Shares no code with the kernels.

For row r and star i with the finite terms t (log lambda_k included), L = logsumexp t and the FULL-DATA membership p: for a
filter the star uses g_f = ((pred_f - obs_f) / sigma_f)^2 / 2, else g_f = 0; t^f = t + g_f, L^f = logsumexp t^f,
w^f = exp(t^f - L^f) -- over both populations at once, which IS the mixture by that leave-out's own population weights --;
the pivot c_f = obs_f where sigma_f > 0, else 0; d_f = pred_f - c_f;
    x = (1, p, then per filter  p sum w^f d_f,  p sum w^f d_f^2,  p l_f),    l_f = (L - L^f) - log(sigma_f sqrt(2 pi)),
l_f = 0 for an unused filter.  A row outside the grid, and a star with no finite term, contribute nothing.  star_loo adds the
rows in ascending order; row_loo[r] = (sum_i p_i, then per filter over the stars with sigma > 0:  N = sum p,
R = -sum x[2+3f] / sigma, C = sum x[3+3f] / sigma^2, W = sum p / sigma^2, D = -sum x[2+3f] / sigma^2, E = sum x[4+3f]), the
stars in ascending order.

Also the two derived tables (star_table, filter_table) restated with numpy, the non-vacuity figures, and six MUTATIONS
(keyword flags) that the comparators of tests/loo_check.py must reject."""
import numpy as np
from scipy.special import logsumexp

import moments_ref as mr
import resid_ref as rr
from base_amd import abi

STAR_MUTATIONS = ("in_sample", "full_pruning", "no_norm", "no_half", "full_pop_weights")
ROW_MUTATIONS = ("count_unused",)
LOG_SQRT_2PI = 0.5 * np.log(2.0 * np.pi)


def ncol(nf):
    return 2 + 3 * nf


def leave_out_terms(cl, i, t, mags, no_half=False):
    """(g [nodes, nf], t^f [nodes, nf]) of one star."""
    obs, sig = np.asarray(cl["obs"], dtype=np.float64)[i], np.asarray(cl["sigma"], dtype=np.float64)[i]
    used = sig > 0
    z = np.where(used[None, :], (mags - obs[None, :]) / np.where(used, sig, 1.0)[None, :], 0.0)
    g = (1.0 if no_half else 0.5) * z * z
    return g, t[:, None] + g


def increments(pack_d, cl, par, n_pops, K, n_q, nodes=None, in_sample=False, full_pruning=False, no_norm=False, no_half=False,
               full_pop_weights=False):
    """(x, bound, absx), each [star, 2 + 3 nf], of one parameter row.  bound: what one dropped unit of weight can move an entry
    by (1 for MEMBER, max |d_f| and max d_f^2 over the star's nodes for the sums, |l_f| + 2 for p l_f: the membership moves by
    one unit and each of L, L^f by one, 0 for ROWS); absx: the scale of an entry's rounding (p sum w^f |d_f| in the
    first-moment columns, p max(1, |L|, |L^f|) in the density columns, |x| elsewhere).  The keyword flags are five of the
    MUTATIONS."""
    nf = pack_d["n_filt"]
    n = len(cl["mass1"])
    x, bound, absx = np.zeros((n, ncol(nf))), np.zeros((n, ncol(nf))), np.zeros((n, ncol(nf)))
    if nodes is None:
        nodes = mr.star_nodes(pack_d, cl, par, n_pops, K, n_q)
    if nodes is None:
        return x, bound, absx
    c = rr.pivots(cl)
    sig = np.asarray(cl["sigma"], dtype=np.float64)
    mags = rr.node_mags(pack_d, cl, par, nodes)
    for i in range(n):
        if mags[i] is None:
            continue
        t, _, _, k = nodes[i]
        w, L = mr.weights(nodes[i])
        p = mr.membership(cl, i, L)
        d = mags[i] - c[i][None, :]
        g, tf = leave_out_terms(cl, i, t, mags[i], no_half)
        Lf = logsumexp(tf, axis=0)
        wf = np.exp(tf - Lf[None, :])
        if in_sample:
            wf = np.repeat(w[:, None], nf, axis=1)
        if full_pruning:                                   # the leave-out sums over the nodes the full-data pruning keeps
            kept = np.where((t > t.max() - 40.0)[:, None], tf, -np.inf)
            Lf = logsumexp(kept, axis=0)
            wf = np.exp(kept - Lf[None, :])
        if full_pop_weights and n_pops == 2:               # each population's own leave-out mean, mixed by the FULL-DATA weights
            wk = np.array([w[k == q].sum() for q in range(2)])
            mix = np.zeros_like(wf)
            for q in range(2):
                s = k == q
                if s.any():
                    mix[s] = wk[q] * wf[s] / wf[s].sum(axis=0)[None, :]
            wf = mix
        used = sig[i] > 0
        lpd = np.where(used, (L - Lf) - (0.0 if no_norm else 1.0) * (np.log(np.where(used, sig[i], 1.0)) + LOG_SQRT_2PI), 0.0)
        x[i, 0], x[i, 1] = 1.0, p
        x[i, 2::3] = p * (wf * d).sum(axis=0)
        x[i, 3::3] = p * (wf * d * d).sum(axis=0)
        x[i, 4::3] = p * lpd
        bound[i, 1] = 1.0
        bound[i, 2::3] = np.abs(d).max(axis=0)
        bound[i, 3::3] = (d * d).max(axis=0)
        bound[i, 4::3] = np.abs(lpd) + 2.0
        absx[i] = np.abs(x[i])
        absx[i, 2::3] = p * (wf * np.abs(d)).sum(axis=0)
        absx[i, 4::3] = p * np.maximum(1.0, np.maximum(abs(L), np.abs(Lf)))
    return x, bound, absx


def all_increments(pack_d, cl, rows, n_pops, K, n_q, nodes_by_row=None, **kw):
    """(x, bound, absx), each [row, star, 2 + 3 nf]"""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
    parts = [increments(pack_d, cl, par, n_pops, K, n_q, nodes=None if nodes_by_row is None else nodes_by_row[r], **kw)
             for r, par in enumerate(rows)]
    return tuple(np.stack([p[k] for p in parts]) for k in range(3))


def accumulate(x, start=None):
    """star_loo: the rows' increments added in ascending row order."""
    acc = np.zeros(x.shape[1:]) if start is None else np.array(start, dtype=np.float64)
    for xr in x:
        acc = acc + xr
    return acc


def row_sums(x, cl, count_unused=False):
    """row_loo [row, 1 + 6 nf]: the stars added in ascending order.  count_unused: one of the MUTATIONS (an unused filter
    counted with sigma = 1)."""
    sig = np.asarray(cl["sigma"], dtype=np.float64)
    n_rows, n, nc = x.shape
    nf = (nc - 2) // 3
    out = np.zeros((n_rows, 1 + 6 * nf))
    for r in range(n_rows):
        a = np.zeros(1 + 6 * nf)
        for i in range(n):
            p = x[r, i, 1]
            a[0] = a[0] + p
            for f in range(nf):
                s = sig[i, f]
                if not s > 0:
                    if not count_unused:
                        continue
                    s = 1.0
                a[1 + 6 * f] = a[1 + 6 * f] + p
                a[2 + 6 * f] = a[2 + 6 * f] - x[r, i, 2 + 3 * f] / s
                a[3 + 6 * f] = a[3 + 6 * f] + x[r, i, 3 + 3 * f] / s ** 2
                a[4 + 6 * f] = a[4 + 6 * f] + p / s ** 2
                a[5 + 6 * f] = a[5 + 6 * f] - x[r, i, 2 + 3 * f] / s ** 2
                a[6 + 6 * f] = a[6 + 6 * f] + x[r, i, 4 + 3 * f]
        out[r] = a
    return out


def reference(pack_d, cl, rows, n_pops, K, n_q, nodes_by_row=None, **mutation):
    """(star_loo, row_loo, x, bound, absx) of the rows."""
    star_kw = {k: v for k, v in mutation.items() if k in STAR_MUTATIONS}
    row_kw = {k: v for k, v in mutation.items() if k in ROW_MUTATIONS}
    x, bound, absx = all_increments(pack_d, cl, rows, n_pops, K, n_q, nodes_by_row, **star_kw)
    return accumulate(x), row_sums(x, cl, **row_kw), x, bound, absx


# ---- what makes the leave-outs a problem of their own: figures of one row ---------------------------------------------------
def non_vacuity(pack_d, cl, par, n_pops, K, n_q, nodes=None):
    """dict of one row's figures: pairs = (star, used filter) pairs of the stars with nodes; shifted = pairs whose leave-out
    prediction differs from the in-sample one by more than 1e-3 mag (max_shift: the largest); promoted = pairs whose largest
    leave-out term lies more than 40 e-folds above the largest full term (max_promotion: by how much, and `promoted_pairs`
    lists them); revived = nodes the full-data pruning (40 e-folds below the largest term) drops although a leave-out keeps
    them within 40 e-folds of its own largest term, counted once per leave-out sum they take part in."""
    if nodes is None:
        nodes = mr.star_nodes(pack_d, cl, par, n_pops, K, n_q)
    mags = rr.node_mags(pack_d, cl, par, nodes)
    sig = np.asarray(cl["sigma"], dtype=np.float64)
    out = dict(pairs=0, shifted=0, max_shift=0.0, promoted=0, max_promotion=0.0, revived=0, promoted_pairs=[])
    for i in range(len(nodes)):
        if mags[i] is None:
            continue
        t = nodes[i][0]
        w, _ = mr.weights(nodes[i])
        _, tf = leave_out_terms(cl, i, t, mags[i])
        wf = np.exp(tf - logsumexp(tf, axis=0)[None, :])
        used = sig[i] > 0
        shift = np.abs((wf * mags[i]).sum(axis=0) - (w[:, None] * mags[i]).sum(axis=0))[used]
        prom = (tf.max(axis=0) - t.max())[used]
        out["pairs"] += int(used.sum())
        out["shifted"] += int((shift > 1e-3).sum())
        out["promoted"] += int((prom > 40).sum())
        out["promoted_pairs"] += [(i, int(f)) for f in np.flatnonzero(used)[prom > 40]]
        if used.any():
            out["max_shift"] = max(out["max_shift"], float(shift.max()))
            out["max_promotion"] = max(out["max_promotion"], float(prom.max()))
        dropped = t <= t.max() - 40.0
        kept_out = tf[:, used] > tf[:, used].max(axis=0)[None, :] - 40.0
        out["revived"] += int((dropped[:, None] & kept_out).sum())
    return out


# ---- the derived tables -----------------------------------------------------------------------------------------------------
STAR_COLUMNS = ("looMag", "looSd", "resid", "z", "lpd")
FILTER_COLUMNS = ("nRows",) + tuple(q + "_" + s for q in ("meanZ", "chi2", "offset", "lpd") for s in ("mean", "sd", "p16", "p50", "p84"))


def star_table(acc, cl):
    """[star, 2 + 5 nf]: rows, member, then per filter looMag = c + acc[2+3f] / acc[1], looSd = sqrt(max(0, between-node
    variance)), resid = obs - looMag, z = resid / sqrt(sigma^2 + variance) (variance floored at 0), lpd = acc[4+3f] / acc[1];
    resid, z and lpd are 0 for an unused filter, everything past `rows` is 0 without membership weight.  Stated independently
    of b9h_loo_table."""
    acc = np.asarray(acc, dtype=np.float64)
    obs, sig = np.asarray(cl["obs"], dtype=np.float64), np.asarray(cl["sigma"], dtype=np.float64)
    n, nf = obs.shape
    used = sig > 0
    c = np.where(used, obs, 0.0)
    out = np.zeros((n, 2 + 5 * nf))
    out[:, 0] = acc[:, 0]
    live = acc[:, 0] > 0
    out[live, 1] = acc[live, 1] / acc[live, 0]
    mem = acc[:, 1] > 0
    den = np.where(mem, acc[:, 1], 1.0)[:, None]
    m1, m2, lp = acc[:, 2::3] / den, acc[:, 3::3] / den, acc[:, 4::3] / den
    var = np.maximum(0.0, m2 - m1 ** 2)
    mem = mem[:, None]
    pred = np.where(mem, c + m1, 0.0)
    out[:, 2::5] = pred
    out[:, 3::5] = np.where(mem, np.sqrt(var), 0.0)
    out[:, 4::5] = np.where(mem & used, obs - pred, 0.0)
    out[:, 5::5] = np.where(mem & used, (obs - pred) / np.sqrt(np.where(used, sig, 1.0) ** 2 + var), 0.0)
    out[:, 6::5] = np.where(mem & used, lp, 0.0)
    return out


def filter_table(row_loo, nf):
    """[nf, 21] (FILTER_COLUMNS): over the rows with N_f > 0 the mean, population sd and 16th / 50th / 84th percentiles
    (np.percentile's default) of R_f / N_f, C_f / N_f, D_f / W_f and E_f / N_f."""
    rl = np.asarray(row_loo, dtype=np.float64).reshape(-1, 1 + 6 * nf)
    out = np.zeros((nf, 21))
    for f in range(nf):
        N, R, Cc, W, D, E = (rl[:, 1 + 6 * f + k] for k in range(6))
        use = N > 0
        out[f, 0] = use.sum()
        if not use.any():
            continue
        with np.errstate(invalid="ignore", divide="ignore"):
            qs = (R[use] / N[use], Cc[use] / N[use], np.where(W[use] > 0, D[use] / np.where(W[use] > 0, W[use], 1.0), 0.0), E[use] / N[use])
        for k, v in enumerate(qs):
            out[f, 1 + 5 * k] = v.mean()
            out[f, 2 + 5 * k] = v.std()
            out[f, 3 + 5 * k:6 + 5 * k] = np.percentile(v, [16, 50, 84])
    return out
