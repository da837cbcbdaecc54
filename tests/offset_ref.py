"""numpy statement of b9_star_offset (tests only): the per-star offset increments of every (row, star), built on
moments_ref.star_nodes (terms, masses, ratios, populations of every finite node), moments_ref.weights, moments_ref.membership
and resid_ref.node_mags (the node magnitudes).  Shares no code with the kernels.

A direction is a vector k[f] over the filters and a prior width tau.  For row r and star i with the finite terms t (log lambda_k
included), L = logsumexp t and the FULL-DATA membership p:  c_f = k_f / sigma_f for a filter the star uses, else 0;
C = sum c_f^2;  V = 1 / (C + tau^-2);  per node  z_f = (pred_f - obs_f) / sigma_f (0 for an unused filter),  B = -sum_f c_f z_f,
mu = V B,  g = V B^2 / 2,  t' = t + g;  L' = logsumexp t' and w' = exp(t' - L') -- over both populations at once, which IS the
mixture by that direction's own population weights --;
    x = (1, p, then per direction  p sum w' mu,  p sum w' mu^2,  p ((L' - L) - log1p(C tau^2) / 2)),
exact zeros in the three columns of a direction with C = 0.  A row outside the grid, and a star with no finite term, contribute
nothing.  star_off adds the rows in ascending order; row_off[r] = (sum_i p_i, then per direction over the stars with C > 0:
N = sum p, M1 = sum x[2+3j], M2 = sum (x[3+3j] + p V), E = sum x[4+3j]), the stars in ascending order.

Also the named directions, the two derived tables (star_table, dist_table) restated with numpy, the non-vacuity figures, and
eight MUTATIONS (keyword flags) that the comparators of tests/offset_check.py must reject."""
import numpy as np
from scipy.special import logsumexp

import moments_ref as mr
import resid_ref as rr
from base_amd import abi

STAR_MUTATIONS = ("no_boost", "full_pruning", "no_half", "no_prior", "no_occam", "full_pop_weights")
ROW_MUTATIONS = ("no_pv", "count_zero")


def ncol(nd):
    return 2 + 3 * nd


def direction(pack_d, name):
    """k[f] of a named direction: `absorption` (the pack's absorption coefficients: more dust at the same true distance),
    `distance` (1 in every filter), `filter:<index>` (a unit vector)."""
    nf = pack_d["n_filt"]
    if name == "absorption":
        return np.array(pack_d["abs_coeff"], dtype=np.float64)[:nf].copy()
    if name == "distance":
        return np.ones(nf)
    if name.startswith("filter:"):
        k = np.zeros(nf)
        k[int(name.split(":")[1])] = 1.0
        return k
    raise ValueError(name)


def directions(pack_d, names):
    return np.stack([direction(pack_d, n) if isinstance(n, str) else np.asarray(n, dtype=np.float64) for n in names])


def star_cv(cl, i, k, tau, no_prior=False):
    """(c [nf], C, V) of star i for one direction."""
    sig = np.asarray(cl["sigma"], dtype=np.float64)[i]
    used = sig > 0
    c = np.where(used, k / np.where(used, sig, 1.0), 0.0)
    C = float((c * c).sum())
    if no_prior:
        return c, C, (1.0 / C if C > 0 else 0.0)
    return c, C, 1.0 / (C + 1.0 / (tau * tau))          # (1 / (tau tau): a power of two in tau scales it exactly)


def all_cv(cl, ks, taus):
    """(C, V), each [star, direction]."""
    n = len(cl["mass1"])
    C, V = np.zeros((n, len(ks))), np.zeros((n, len(ks)))
    for i in range(n):
        for j, (k, tau) in enumerate(zip(ks, taus)):
            _, C[i, j], V[i, j] = star_cv(cl, i, k, tau)
    return C, V


def boosted_terms(cl, i, t, mags, k, tau, no_half=False, no_prior=False):
    """(mu [nodes], g [nodes], t' [nodes], C, V) of one star and direction."""
    obs, sig = np.asarray(cl["obs"], dtype=np.float64)[i], np.asarray(cl["sigma"], dtype=np.float64)[i]
    used = sig > 0
    c, C, V = star_cv(cl, i, k, tau, no_prior)
    z = np.where(used[None, :], (mags - obs[None, :]) / np.where(used, sig, 1.0)[None, :], 0.0)
    B = -(z * c[None, :]).sum(axis=1)
    mu = V * B
    g = (1.0 if no_half else 0.5) * V * B * B
    return mu, g, t + g, C, V


def increments(pack_d, cl, par, n_pops, K, n_q, ks, taus, nodes=None, no_boost=False, full_pruning=False, no_half=False, no_prior=False,
               no_occam=False, full_pop_weights=False):
    """(x, bound, absx), each [star, 2 + 3 D], of one parameter row.  bound: what one dropped unit of weight can move an entry
    by (1 for MEMBER, max |mu| and max mu^2 over the star's nodes for the sums, |logBF| + 2 for the last column: the membership
    moves by one unit and each of L, L' by one; 0 for ROWS); absx: the scale of an entry's rounding (p sum w' |mu| in the
    first-moment columns, p max(1, |L|, |L'|) in the last, |x| elsewhere).  The keyword flags are six of the MUTATIONS."""
    nd = len(ks)
    n = len(cl["mass1"])
    x, bound, absx = np.zeros((n, ncol(nd))), np.zeros((n, ncol(nd))), np.zeros((n, ncol(nd)))
    if nodes is None:
        nodes = mr.star_nodes(pack_d, cl, par, n_pops, K, n_q)
    if nodes is None:
        return x, bound, absx
    mags = rr.node_mags(pack_d, cl, par, nodes)
    for i in range(n):
        if mags[i] is None:
            continue
        t, _, _, pop = nodes[i]
        w, L = mr.weights(nodes[i])
        p = mr.membership(cl, i, L)
        x[i, 0], x[i, 1] = 1.0, p
        bound[i, 1] = 1.0
        absx[i, :2] = np.abs(x[i, :2])
        for j, (k, tau) in enumerate(zip(ks, taus)):
            mu, g, tb, C, V = boosted_terms(cl, i, t, mags[i], k, tau, no_half, no_prior)
            if not C > 0:
                continue
            if no_boost:
                tb = t
            Lb = logsumexp(tb)
            wb = np.exp(tb - Lb)
            if full_pruning:                               # the offset sums over the nodes the full-data pruning keeps
                kept = np.where(t > t.max() - 40.0, tb, -np.inf)
                Lb = logsumexp(kept)
                wb = np.exp(kept - Lb)
            if full_pop_weights and n_pops == 2:           # each population's own offset mean, mixed by the FULL-DATA weights
                mix = np.zeros_like(wb)
                for q in range(2):
                    s = pop == q
                    if s.any() and wb[s].sum() > 0:
                        mix[s] = w[s].sum() * wb[s] / wb[s].sum()
                wb = mix
            occ = 0.0 if no_occam else 0.5 * np.log1p(C * tau * tau)
            lbf = (Lb - L) - occ
            x[i, 2 + 3 * j] = p * (wb * mu).sum()
            x[i, 3 + 3 * j] = p * (wb * mu * mu).sum()
            x[i, 4 + 3 * j] = p * lbf
            bound[i, 2 + 3 * j] = np.abs(mu).max()
            bound[i, 3 + 3 * j] = (mu * mu).max()
            bound[i, 4 + 3 * j] = abs(lbf) + 2.0
            absx[i, 2 + 3 * j] = p * (wb * np.abs(mu)).sum()
            absx[i, 3 + 3 * j] = abs(x[i, 3 + 3 * j])
            absx[i, 4 + 3 * j] = p * max(1.0, abs(L), abs(Lb))
    return x, bound, absx


def all_increments(pack_d, cl, rows, n_pops, K, n_q, ks, taus, nodes_by_row=None, **kw):
    """(x, bound, absx), each [row, star, 2 + 3 D]"""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
    parts = [increments(pack_d, cl, par, n_pops, K, n_q, ks, taus, nodes=None if nodes_by_row is None else nodes_by_row[r], **kw)
             for r, par in enumerate(rows)]
    return tuple(np.stack([p[q] for p in parts]) for q in range(3))


def accumulate(x, start=None):
    """star_off: the rows' increments added in ascending row order."""
    acc = np.zeros(x.shape[1:]) if start is None else np.array(start, dtype=np.float64)
    for xr in x:
        acc = acc + xr
    return acc


def row_sums(x, cl, ks, taus, no_pv=False, count_zero=False):
    """row_off [row, 1 + 4 D]: the stars added in ascending order.  no_pv, count_zero: two of the MUTATIONS (M2 without p V;
    the stars a direction does not touch counted in its sums)."""
    C, V = all_cv(cl, ks, taus)
    n_rows, n, nc = x.shape
    nd = (nc - 2) // 3
    out = np.zeros((n_rows, 1 + 4 * nd))
    for r in range(n_rows):
        a = np.zeros(1 + 4 * nd)
        for i in range(n):
            p = x[r, i, 1]
            a[0] = a[0] + p
            for j in range(nd):
                if not (C[i, j] > 0 or count_zero):
                    continue
                a[1 + 4 * j] = a[1 + 4 * j] + p
                a[2 + 4 * j] = a[2 + 4 * j] + x[r, i, 2 + 3 * j]
                a[3 + 4 * j] = a[3 + 4 * j] + (x[r, i, 3 + 3 * j] + (0.0 if no_pv else p * V[i, j]))
                a[4 + 4 * j] = a[4 + 4 * j] + x[r, i, 4 + 3 * j]
        out[r] = a
    return out


def reference(pack_d, cl, rows, n_pops, K, n_q, ks, taus, nodes_by_row=None, **mutation):
    """(star_off, row_off, x, bound, absx) of the rows."""
    star_kw = {q: v for q, v in mutation.items() if q in STAR_MUTATIONS}
    row_kw = {q: v for q, v in mutation.items() if q in ROW_MUTATIONS}
    x, bound, absx = all_increments(pack_d, cl, rows, n_pops, K, n_q, ks, taus, nodes_by_row, **star_kw)
    return accumulate(x), row_sums(x, cl, ks, taus, **row_kw), x, bound, absx


# ---- what makes the offsets a problem of their own: figures of one row ------------------------------------------------------
def non_vacuity(pack_d, cl, par, n_pops, K, n_q, k, tau, nodes=None):
    """dict of one row's figures for one direction: stars = the stars with nodes the direction touches; shifted = those whose
    offset weights differ from the full-data ones by more than 1e-3 in L1; promoted = those whose largest boosted term lies more
    than 40 e-folds above the largest full term (max_promotion: by how much); revived = nodes the full-data pruning (40 e-folds
    below the largest term) drops although the offset sum keeps them within 40 e-folds of its own largest term."""
    if nodes is None:
        nodes = mr.star_nodes(pack_d, cl, par, n_pops, K, n_q)
    mags = rr.node_mags(pack_d, cl, par, nodes)
    out = dict(stars=0, shifted=0, promoted=0, max_promotion=0.0, revived=0, max_rho=0.0)
    for i in range(len(nodes)):
        if mags[i] is None:
            continue
        t = nodes[i][0]
        w, _ = mr.weights(nodes[i])
        _, _, tb, C, V = boosted_terms(cl, i, t, mags[i], k, tau)
        if not C > 0:
            continue
        wb = np.exp(tb - logsumexp(tb))
        prom = tb.max() - t.max()
        out["stars"] += 1
        out["shifted"] += int(np.abs(wb - w).sum() > 1e-3)
        out["promoted"] += int(prom > 40)
        out["max_promotion"] = max(out["max_promotion"], float(prom))
        out["revived"] += int(((t <= t.max() - 40.0) & (tb > tb.max() - 40.0)).sum())
        out["max_rho"] = max(out["max_rho"], C * V)
    return out


# ---- the derived tables -----------------------------------------------------------------------------------------------------
STAR_COLUMNS = ("mean", "sd", "z", "logBF")
DIST_COLUMNS = ("nRows",) + tuple(q + "_" + s for q in ("mean", "rms", "logBF") for s in ("mean", "sd", "p16", "p50", "p84"))


def star_table(acc, cl, ks, taus):
    """[star, 2 + 4 D]: rows, member, then per direction mean = acc[2+3j] / acc[1], sd = sqrt(max(0, acc[3+3j] / acc[1] -
    mean^2) + V), z = mean / sd, logBF = acc[4+3j] / acc[1]; everything past `rows` is 0 without membership weight.  Stated
    independently of b9h_offset_table."""
    acc = np.asarray(acc, dtype=np.float64)
    n = acc.shape[0]
    nd = len(ks)
    _, V = all_cv(cl, ks, taus)
    out = np.zeros((n, 2 + 4 * nd))
    out[:, 0] = acc[:, 0]
    live = acc[:, 0] > 0
    out[live, 1] = acc[live, 1] / acc[live, 0]
    mem = acc[:, 1] > 0
    den = np.where(mem, acc[:, 1], 1.0)[:, None]
    m1, m2, lb = acc[:, 2::3] / den, acc[:, 3::3] / den, acc[:, 4::3] / den
    sd = np.sqrt(np.maximum(0.0, m2 - m1 ** 2) + V)
    mem = mem[:, None]
    out[:, 2::4] = np.where(mem, m1, 0.0)
    out[:, 3::4] = np.where(mem, sd, 0.0)
    out[:, 4::4] = np.where(mem, m1 / sd, 0.0)
    out[:, 5::4] = np.where(mem, lb, 0.0)
    return out


def dist_table(row_off, nd):
    """[D, 16] (DIST_COLUMNS): over the rows with N > 0 the mean, population sd and 16th / 50th / 84th percentiles
    (np.percentile's default) of M1 / N, sqrt(M2 / N) and E / N."""
    ro = np.asarray(row_off, dtype=np.float64).reshape(-1, 1 + 4 * nd)
    out = np.zeros((nd, 16))
    for j in range(nd):
        N, M1, M2, E = (ro[:, 1 + 4 * j + q] for q in range(4))
        use = N > 0
        out[j, 0] = use.sum()
        if not use.any():
            continue
        qs = (M1[use] / N[use], np.sqrt(M2[use] / N[use]), E[use] / N[use])
        for q, v in enumerate(qs):
            out[j, 1 + 5 * q] = v.mean()
            out[j, 2 + 5 * q] = v.std()
            out[j, 3 + 5 * q:6 + 5 * q] = np.percentile(v, [16, 50, 84])
    return out
