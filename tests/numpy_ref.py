"""A third, numpy-only statement of the given-mass log-posterior (tests only).

Built on base_amd.synth.forward_mags; shares no code with oracle/b9_oracle.c or the kernels.
"""
import numpy as np
from scipy.special import erfc, logsumexp

from base_amd import abi, synth

MF_MU, MF_SIGMA, LN10 = -1.02, 0.67729, np.log(10.0)


def log_mass_norm(m_wd_up):
    Phi = lambda x: 0.5 * erfc(-x / np.sqrt(2.0))
    zup, zlow = (np.log10(m_wd_up) - MF_MU) / MF_SIGMA, (-1.0 - MF_MU) / MF_SIGMA
    return np.log(1.0 / (MF_SIGMA * np.sqrt(2 * np.pi) * (Phi(zup) - Phi(zlow))))


def log_prior_mass(m, m_wd_up):
    z = (np.log10(m) - MF_MU) / MF_SIGMA
    return log_mass_norm(m_wd_up) - 0.5 * z * z - np.log(m) - np.log(LN10)


def log_prior_cluster(priors, par, n_pops):
    if not (priors.log_age_min <= par[abi.P_LOGAGE] <= priors.log_age_max) or par[abi.P_ABS] < 0:
        return -np.inf
    if n_pops == 2 and not (0.0 <= par[abi.P_LAMBDA] <= 1.0):
        return -np.inf
    lp = 0.0
    for k in range(abi.B9_NPARAM):
        if k == abi.P_LOGAGE or (n_pops < 2 and k in (abi.P_Y2, abi.P_LAMBDA)):
            continue
        if priors.var[k] > 0:
            lp -= 0.5 * (par[k] - priors.mean[k]) ** 2 / priors.var[k]
    return lp


def star_loglike(pack_d, cl, par, pop=0):
    pred = synth.forward_mags(pack_d, par, cl["mass1"], cl["mass_ratio"], cl["wd_type"], pop=pop)
    sig = np.asarray(cl["sigma"])
    used = sig > 0
    var = np.where(used, sig ** 2, 1.0)
    term = np.where(used, -0.5 * (np.log(2 * np.pi * var) + (pred - cl["obs"]) ** 2 / var), 0.0)
    return log_prior_mass(cl["mass1"], pack_d["m_wd_up"]) + term.sum(axis=1)


def logpost(pack_d, cl, priors, par, n_pops=1):
    """(logpost, perstar) for one parameter row; -inf outside the grid."""
    lp = log_prior_cluster(priors, par, n_pops)
    n = len(cl["mass1"])
    if not np.isfinite(lp):
        return -np.inf, np.full(n, -np.inf)
    try:
        ll = star_loglike(pack_d, cl, par, 0)
        if n_pops == 2:
            llb = star_loglike(pack_d, cl, par, 1)
            lam = par[abi.P_LAMBDA]
            with np.errstate(divide="ignore"):
                ll = logsumexp(np.stack([np.log(lam) + ll, np.log1p(-lam) + llb]), axis=0)
    except ValueError:
        return -np.inf, np.full(n, -np.inf)
    log_fs = -np.sum(np.log(cl["filter_prior_max"] - cl["filter_prior_min"]))
    pm = cl["clust_prior"]
    with np.errstate(divide="ignore"):
        v = logsumexp(np.stack([np.log1p(-pm) + log_fs, np.log(pm) + ll]), axis=0)
    return lp + v.sum(), v


def marg_terms(pack_d, cl, par, K, Q, pop=0):
    """The terms of marg_perstar's sum, kept:  (terms[star, node], mass[node], ratio[node])  with
    terms = log(prior(M1) * dM/Q * prod_f N(obs_f | combined_f, sigma_f^2))  over every primary node (K sub-steps per EEP
    interval, left endpoints) and every mass ratio j/Q -- ratio-major: node = j * n_primary + primary.  mass is the node's
    primary mass, ratio its j/Q.  exp(terms - logsumexp(terms)) is the star's posterior over the grid."""
    first, imass, imags = synth.derive_isochrone(pack_d, par[abi.P_LOGAGE], par[abi.P_FEH], par[abi.P_Y2 if pop else abi.P_Y])
    m_nodes, w_nodes = [], []
    for e in range(len(imass) - 1):
        d = imass[e + 1] - imass[e]
        if not d > 0:
            continue
        for s in range(K):
            m_nodes.append(imass[e] + s * (d / K))
            w_nodes.append(d / K / Q)
    m_nodes, w_nodes = np.array(m_nodes), np.array(w_nodes)
    n = len(cl["mass1"])
    sig = np.asarray(cl["sigma"]); used = sig > 0
    var = np.where(used, sig ** 2, 1.0)
    lpm = log_prior_mass(m_nodes, pack_d["m_wd_up"]) + np.log(w_nodes)
    preds = []
    for j in range(Q):
        q = np.full(len(m_nodes), j / Q)
        preds.append(synth.forward_mags(pack_d, par, m_nodes, q, np.zeros(len(m_nodes), int), pop=pop))      # [nodes, nf]
    terms = np.empty((n, Q * len(m_nodes)))
    for i in range(n):
        acc = []
        for pred in preds:
            g = np.where(used[i], -0.5 * (np.log(2 * np.pi * var[i]) + (pred - cl["obs"][i]) ** 2 / var[i]), 0.0).sum(axis=1)
            acc.append(lpm + g)
        terms[i] = np.concatenate(acc)
    return terms, np.tile(m_nodes, Q), np.repeat(np.arange(Q) / Q, len(m_nodes))


def marg_perstar(pack_d, cl, par, K, Q, pop=0):
    """Brute-force numpy statement of the marginalised per-star log-likelihood of MS/RGB-stage stars
    (WD-stage stars: marg_perstar_wd): log sum over primary nodes (K sub-steps per EEP interval, left endpoints) and mass
    ratios j/Q of  prior(M1) * dM/Q * prod_f N(obs_f | combined_f, sigma_f^2).  Independent of the C oracle."""
    terms, _, _ = marg_terms(pack_d, cl, par, K, Q, pop)
    out = np.full(len(terms), -np.inf)
    for i in range(len(terms)):
        out[i] = logsumexp(terms[i])
    return out


def marg_terms_wd(pack_d, cl, par, K, pop=0, n_nodes=None):
    """The terms of marg_perstar_wd's sum, kept:  (terms[star, node], mass[node]),  node j - 1 at M1 = tip + j dM,
    j = 1 .. 8 K (or 1 .. n_nodes, the grid of b9_sample_wd_mass), each star through the WD branch with its own DA / DB
    flag; mass ratio 0.  Rows of other stars: NaN.  (None, None) where the AGB tip is not below M_wd_up."""
    first, imass, imags = synth.derive_isochrone(pack_d, par[abi.P_LOGAGE], par[abi.P_FEH], par[abi.P_Y2 if pop else abi.P_Y])
    tip, steps = imass[-1], n_nodes or 8 * K
    dM = (pack_d["m_wd_up"] - tip) / steps
    if not dM > 0:
        return None, None
    n = len(cl["mass1"])
    m_nodes = tip + dM * np.arange(1, steps + 1)
    lpm = log_prior_mass(m_nodes, pack_d["m_wd_up"]) + np.log(dM)
    sig = np.asarray(cl["sigma"]); used = sig > 0
    var = np.where(used, sig ** 2, 1.0)
    terms = np.full((n, steps), np.nan)
    pred_by_type = {}
    for i in np.nonzero(np.asarray(cl["stage"]) == abi.STAGE_WD)[0]:
        ty = int(cl["wd_type"][i])
        if ty not in pred_by_type:
            pred_by_type[ty] = synth.forward_mags(pack_d, par, m_nodes, np.zeros(steps), np.full(steps, ty, int), pop=pop)
        pred = pred_by_type[ty]
        g = np.where(used[i], -0.5 * (np.log(2 * np.pi * var[i]) + (pred - cl["obs"][i]) ** 2 / var[i]), 0.0).sum(axis=1)
        terms[i] = lpm + g
    return terms, m_nodes


def marg_perstar_wd(pack_d, cl, par, K, pop=0):
    """The same for the catalogue's WD-stage stars: M1 over (AGB tip, M_wd_up] in 8 K equal steps
    (right endpoints tip + j dM, j = 1 .. 8 K), single stars, each through the WD branch of synth.forward_mags with the
    star's own DA / DB flag:  log sum_j prior(M1_j) dM prod_f N(obs_f | wd_f(M1_j), sigma_f^2).  Entries of other stars: NaN."""
    terms, _ = marg_terms_wd(pack_d, cl, par, K, pop)
    wd = np.asarray(cl["stage"]) == abi.STAGE_WD
    out = np.full(len(cl["mass1"]), np.nan)
    if terms is None:
        out[wd] = -np.inf
        return out
    for i in np.nonzero(wd)[0]:
        t = terms[i][np.isfinite(terms[i])]
        out[i] = logsumexp(t) if len(t) else -np.inf
    return out


def marg_logpost(pack_d, cl, priors, par, K, Q, n_pops=1):
    """(logpost, perstar) of the marginalised mode for one parameter row, every stage and one or two populations:
    per star  logaddexp(log(1 - p) + log fs,  log p + [logaddexp over populations of log weight + marginal])."""
    n = len(cl["mass1"])
    lp = log_prior_cluster(priors, par, n_pops)
    if not np.isfinite(lp):
        return -np.inf, np.full(n, -np.inf)
    wd = np.asarray(cl["stage"]) == abi.STAGE_WD
    ll_pop = []
    try:
        for pop in range(n_pops):
            ll = marg_perstar(pack_d, cl, par, K, Q, pop)
            if wd.any():
                ll = np.where(wd, marg_perstar_wd(pack_d, cl, par, K, pop), ll)
            ll_pop.append(ll)
    except ValueError:
        return -np.inf, np.full(n, -np.inf)
    ll = ll_pop[0]
    if n_pops == 2:
        lam = par[abi.P_LAMBDA]
        with np.errstate(divide="ignore"):
            ll = logsumexp(np.stack([np.log(lam) + ll_pop[0], np.log1p(-lam) + ll_pop[1]]), axis=0)
    log_fs = -np.sum(np.log(cl["filter_prior_max"] - cl["filter_prior_min"]))
    pm = cl["clust_prior"]
    with np.errstate(divide="ignore"):
        v = logsumexp(np.stack([np.log1p(-pm) + log_fs, np.log(pm) + ll]), axis=0)
    return lp + v.sum(), v
