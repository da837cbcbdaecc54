"""numpy statement of b9_star_moments (tests only): the eight increments of every (row, star), built from
numpy_ref.marg_terms / marg_terms_wd -- the terms, masses and ratios of every node -- with scipy's logsumexp.  Shares no
code with the kernels or the C oracle.

For row r and star i: the populations' terms are concatenated with log lambda / log(1 - lambda), the finite ones kept,
L = logsumexp, w = exp(t - L); membership p = p_i e^L / (p_i e^L + (1 - p_i) fieldLike) with fieldLike the reciprocal volume
of the filter-prior box; x = (1, p, p sum w M1, p sum w M1^2, p sum w q, p sum w q^2, p sum_{q>0} w, p sum_{k=1} w).  A row
outside the grid, and a star with no finite term, contribute nothing."""
import numpy as np
from scipy.special import logsumexp

import numpy_ref
from base_amd import abi

N = 8
ROWS, MEMBER, M1, M1SQ, Q, QSQ, BINARY, POP1 = range(8)


def star_nodes(pack_d, cl, par, n_pops, K, n_q):
    """Per star: (terms, mass, ratio, pop) over every finite node of every population (log lambda_k included), or None
    for every star when the row lies outside the grid."""
    n = len(cl["mass1"])
    wd = np.asarray(cl["stage"]) == abi.STAGE_WD
    lam = par[abi.P_LAMBDA]
    with np.errstate(divide="ignore"):
        lw = [0.0] if n_pops == 1 else [np.log(lam), np.log1p(-lam)]
    per_pop = []
    from base_amd import synth
    for pop in range(n_pops):                            # (outside the grid: no isochrone)
        if synth.derive_isochrone(pack_d, par[abi.P_LOGAGE], par[abi.P_FEH], par[abi.P_Y2 if pop else abi.P_Y]) is None:
            return None
    try:
        for pop in range(n_pops):
            t, gm, gq = numpy_ref.marg_terms(pack_d, cl, par, K, n_q, pop)
            tw, gw = numpy_ref.marg_terms_wd(pack_d, cl, par, K, pop) if wd.any() else (None, None)
            per_pop.append((t, gm, gq, tw, gw))
    except ValueError:
        return None
    out = []
    for i in range(n):
        ts, ms, qs, ks = [], [], [], []
        for pop, (t, gm, gq, tw, gw) in enumerate(per_pop):
            if wd[i]:
                if tw is None:
                    continue
                ti, mi, qi = tw[i], gw, np.zeros(len(gw))
            else:
                ti, mi, qi = t[i], gm, gq
            ok = np.isfinite(ti + lw[pop])
            ts.append(ti[ok] + lw[pop]); ms.append(mi[ok]); qs.append(qi[ok]); ks.append(np.full(int(ok.sum()), pop))
        if ts:
            out.append((np.concatenate(ts), np.concatenate(ms), np.concatenate(qs), np.concatenate(ks)))
        else:
            out.append((np.empty(0), np.empty(0), np.empty(0), np.empty(0, int)))
    return out


def membership(cl, i, L):
    """p_i e^L / (p_i e^L + (1 - p_i) fieldLike)."""
    log_fs = -np.sum(np.log(np.asarray(cl["filter_prior_max"]) - np.asarray(cl["filter_prior_min"])))
    pm = float(np.asarray(cl["clust_prior"])[i])
    if pm <= 0.0:
        return 0.0
    if pm >= 1.0:
        return 1.0
    a, b = np.log(pm) + L, np.log1p(-pm) + log_fs
    return float(np.exp(a - np.logaddexp(a, b)))


def weights(nodes_i):
    """(w, L) of one star's nodes."""
    t = nodes_i[0]
    L = logsumexp(t)
    return np.exp(t - L), L


def increments(pack_d, cl, par, n_pops, K, n_q, second_moment_power=2, drop_pop_weight=False, nodes=None):
    """x[star, 8] of one parameter row.  second_moment_power / drop_pop_weight: the two MUTATIONS the statistical checks
    must reject (second moments built from M1 instead of M1^2; the population weight log lambda_k left out).  nodes: the
    row's star_nodes, where the caller has them already."""
    n = len(cl["mass1"])
    x = np.zeros((n, N))
    if drop_pop_weight and n_pops == 2:
        par = np.array(par, dtype=np.float64)
        par[abi.P_LAMBDA] = 0.5                              # equal weights: log lambda_k only shifts every term alike
        nodes = None
    if nodes is None:
        nodes = star_nodes(pack_d, cl, par, n_pops, K, n_q)
    if nodes is None:
        return x
    for i in range(n):
        t, m, q, k = nodes[i]
        if len(t) == 0:
            continue
        w, L = weights(nodes[i])
        p = membership(cl, i, L)
        x[i] = [1.0, p, p * np.sum(w * m), p * np.sum(w * m ** second_moment_power), p * np.sum(w * q),
                p * np.sum(w * q ** second_moment_power), p * np.sum(w[q > 0]), p * np.sum(w[k == 1])]
    return x


def accumulate(pack_d, cl, rows, n_pops, K, n_q, **kw):
    """acc[star, 8]: the rows' increments added in ascending row order."""
    acc = np.zeros((len(cl["mass1"]), N))
    for par in np.asarray(rows, dtype=np.float64).reshape(-1, abi.B9_NPARAM):
        acc = acc + increments(pack_d, cl, par, n_pops, K, n_q, **kw)
    return acc


def table(acc):
    """The derived columns (rows, member, mass, massSd, massRatio, massRatioSd, pBinary, pPop2), stated independently of
    b9h_star_table."""
    acc = np.asarray(acc, dtype=np.float64).reshape(-1, N)
    out = np.zeros_like(acc)
    out[:, 0] = acc[:, ROWS]
    live = acc[:, ROWS] > 0
    out[live, 1] = acc[live, MEMBER] / acc[live, ROWS]
    m = acc[:, MEMBER] > 0
    a = acc[m]
    mass, ratio = a[:, M1] / a[:, MEMBER], a[:, Q] / a[:, MEMBER]
    out[m, 2] = mass
    out[m, 3] = np.sqrt(np.maximum(0.0, a[:, M1SQ] / a[:, MEMBER] - mass ** 2))
    out[m, 4] = ratio
    out[m, 5] = np.sqrt(np.maximum(0.0, a[:, QSQ] / a[:, MEMBER] - ratio ** 2))
    out[m, 6] = a[:, BINARY] / a[:, MEMBER]
    out[m, 7] = a[:, POP1] / a[:, MEMBER]
    return out


def skewness(nodes_i):
    """(mean, variance, skewness gamma_1) of the primary mass under one star's node weights."""
    w, _ = weights(nodes_i)
    m = nodes_i[1]
    mu = np.sum(w * m)
    var = np.sum(w * (m - mu) ** 2)
    g1 = np.sum(w * (m - mu) ** 3) / var ** 1.5 if var > 0 else 0.0
    return mu, var, g1


# ---- statistical checks of draws (b9_sample_mass's, or numpy's from the weights above) against a moments table --------------
P_MIN = 1e-7          # every exact binomial test must give at least this
Z_MAX = 6.0           # |z| of a star's mean drawn mass
SKEW_GUARD = 0.3      # a star's mean is tested while |gamma_1| / sqrt(R) stays below this (the normal approximation holds)


def binomial_pvalues(tab, acc, n_binary, n_pop1, n_draws, n_pops):
    """Two-sided exact tests of the counts of ratio > 0 against Binomial(R, pBinary) and of pop == 1 against
    Binomial(R, pPop2), for the stars with membership weight and a probability strictly inside (0, 1)."""
    from scipy.stats import binomtest
    out = []
    for i in np.flatnonzero(np.asarray(acc)[:, MEMBER] > 0):
        for col, k in ((6, n_binary[i]),) + (((7, n_pop1[i]),) if n_pops == 2 else ()):
            pr = float(tab[i, col])
            if 0.0 < pr < 1.0:
                out.append(binomtest(int(k), int(n_draws), pr).pvalue)
    return np.array(out)


def mass_z(tab, mean_drawn, ref_moments, n_draws):
    """z of every guarded star's mean drawn mass against the table's mass, with the REFERENCE's variance; ref_moments:
    per star (mean, variance, gamma_1) of the reference posterior, or None for a star without nodes.  A star whose table
    gives it no spread (massSd == 0) while the reference does is reported as z = inf."""
    z = []
    for i, mo in enumerate(ref_moments):
        if mo is None or not mo[1] > 0 or abs(mo[2]) / np.sqrt(n_draws) > SKEW_GUARD:
            continue
        if not tab[i, 3] > 0:
            z.append(np.inf)
            continue
        z.append((mean_drawn[i] - tab[i, 2]) / np.sqrt(mo[1] / n_draws))
    return np.array(z)


def numpy_draws(nodes, n_draws, seed):
    """n_draws independent nodes per star from the reference weights: (mean mass, count of ratio > 0, count of pop == 1)."""
    rng = np.random.default_rng(seed)
    n = len(nodes)
    mean_m, n_bin, n_p1 = np.zeros(n), np.zeros(n, int), np.zeros(n, int)
    for i, nd in enumerate(nodes):
        if len(nd[0]) == 0:
            continue
        w, _ = weights(nd)
        idx = rng.choice(len(w), size=n_draws, p=w / w.sum())
        mean_m[i], n_bin[i], n_p1[i] = nd[1][idx].mean(), int((nd[2][idx] > 0).sum()), int((nd[3][idx] == 1).sum())
    return mean_m, n_bin, n_p1
