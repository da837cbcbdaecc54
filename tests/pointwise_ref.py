"""numpy statement of b9_pointwise and of the modelScore tables (tests only).  Shares no code with the kernels or the host
library: v from moments_ref.star_nodes plus the field term, the accumulate recurrence in the stated order, the top-T, the row
sums, and the WAIC / PSIS-LOO arithmetic -- the latter on the FULL [rows] vector of a star (the non-tail sum formed directly),
not through acc / tail.

For row r and star i:  L = logsumexp over the star's finite nodes of every population (log lambda_k included; no node: -inf),
v = logaddexp(log p_i + L, log(1 - p_i) + log fs) with fs the reciprocal volume of the filter-prior box.  A star with no node has
v = the field term (-inf at p_i = 1) and COUNTS; a row outside the grid contributes nothing to any star."""
import math

import numpy as np
from scipy.special import logsumexp

import moments_ref as mr
from base_amd import abi

N = 8
ROWS, NINF, VMAX, SPOS, RMAX, SNEG, MEAN, M2 = range(8)
T_ROWS, T_NINF, T_LPPD, T_PWAIC, T_ELPD_WAIC, T_ELPD_IS, T_K, T_ELPD_LOO, T_PLOO = range(9)


# ---- v ----------------------------------------------------------------------------------------------------------------------
def field_term(cl, i):
    log_fs = -np.sum(np.log(np.asarray(cl["filter_prior_max"]) - np.asarray(cl["filter_prior_min"])))
    pm = float(np.asarray(cl["clust_prior"])[i])
    return -np.inf if pm >= 1.0 else math.log1p(-pm) + log_fs


def values(pack_d, cl, par, n_pops, K, n_q, drop_field=False, drop_pop_weight=False, nodes=None):
    """(v [star], live [star]: the star has a node) of one parameter row, or None for a row outside the grid.  drop_field /
    drop_pop_weight: two MUTATIONS the comparators must reject (the field term left out; log lambda_k left out of every term)."""
    if nodes is None:                                    # (nodes: the row's moments_ref.star_nodes, where the caller has them)
        nodes = mr.star_nodes(pack_d, cl, par, n_pops, K, n_q)
    if nodes is None:
        return None
    n = len(cl["mass1"])
    v, live = np.empty(n), np.zeros(n, bool)
    with np.errstate(divide="ignore"):
        lw = np.array([0.0] if n_pops == 1 else [np.log(par[abi.P_LAMBDA]), np.log1p(-par[abi.P_LAMBDA])])
    for i in range(n):
        t, _, _, k = nodes[i]
        if drop_pop_weight and len(t):
            t = t - lw[k]
        live[i] = len(t) > 0
        L = logsumexp(t) if len(t) else -np.inf
        pm = float(np.asarray(cl["clust_prior"])[i])
        with np.errstate(divide="ignore"):
            a = (np.log(pm) if pm > 0 else -np.inf) + L
        b = -np.inf if drop_field else field_term(cl, i)
        v[i] = np.logaddexp(a, b) if max(a, b) > -np.inf else -np.inf
    return v, live


def v_matrix(pack_d, cl, rows, n_pops, K, n_q, **mutation):
    """(V [row, star] -- NaN in a row outside the grid --, inside [row], live [row, star])."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
    n = len(cl["mass1"])
    V, inside, live = np.full((len(rows), n), np.nan), np.zeros(len(rows), bool), np.zeros((len(rows), n), bool)
    for r, par in enumerate(rows):
        got = values(pack_d, cl, par, n_pops, K, n_q, **mutation)
        if got is not None:
            V[r], live[r] = got
            inside[r] = True
    return V, inside, live


# ---- the reducers -----------------------------------------------------------------------------------------------------------
def accumulate(V, inside=None, acc=None, skip=None, m2_from_old_mean=False):
    """acc [star, 8] after the rows of V in ascending order, by the stated recurrence.  skip [row, star]: (row, star) pairs left
    out altogether, and m2_from_old_mean: M2 += (v - mean_old)^2 -- two MUTATIONS."""
    V = np.asarray(V, dtype=np.float64)
    n_rows, n = V.shape
    inside = np.ones(n_rows, bool) if inside is None else inside
    acc = np.zeros((n, N)) if acc is None else np.array(acc, dtype=np.float64)
    for r in range(n_rows):
        if not inside[r]:
            continue
        for i in range(n):
            if skip is not None and skip[r, i]:
                continue
            a, v = acc[i], float(V[r, i])
            k = a[ROWS] - a[NINF]
            a[ROWS] += 1.0
            if v == -np.inf:
                a[NINF] += 1.0
                continue
            if k == 0:
                a[VMAX:] = (v, 1.0, -v, 1.0, v, 0.0)
                continue
            for mx, s, x in ((VMAX, SPOS, v), (RMAX, SNEG, -v)):
                if x > a[mx]:
                    a[s] = a[s] * math.exp(a[mx] - x) + 1.0
                    a[mx] = x
                else:
                    a[s] += math.exp(x - a[mx])
            d = v - a[MEAN]
            a[MEAN] += d / (k + 1.0)
            a[M2] += d * d if m2_from_old_mean else d * (v - a[MEAN])
    return acc


def top_tail(V, inside, T, ascending=False):
    """tail [star, T]: the T largest r = -v among the star's finite rows, descending, padded with -inf (ascending: a MUTATION)."""
    V = np.asarray(V, dtype=np.float64)
    n = V.shape[1]
    out = np.full((n, T), -np.inf)
    for i in range(n):
        r = -V[inside, i]
        r = np.sort(r[np.isfinite(r)])[::-1][:T]
        out[i, :len(r)] = r[::-1] if ascending else r
    return out


def row_sums(V, inside):
    """row_lpd [row]: the stars' values added in ascending order, one add each; -inf for a row outside the grid."""
    out = np.full(len(V), -np.inf)
    for r in np.flatnonzero(inside):
        a = 0.0
        for x in V[r]:
            a = a + float(x)
        out[r] = a
    return out


# ---- WAIC and PSIS-LOO of one star, on its full vector ----------------------------------------------------------------------
def tail_length(n_f, n_t):
    return min(int(n_f // 5), int(math.ceil(3.0 * math.sqrt(n_f))), n_t - 1)


def gpd_fit(x, shrink=True):
    """Zhang & Stephens' estimate (k, sigma) of the generalised Pareto distribution for the ascending sample x > 0 (x[-1] > 0),
    with the weakly informative prior on k (shrink=False: left out, a MUTATION)."""
    n = len(x)
    m = 30 + int(math.floor(math.sqrt(n)))
    x_star = x[int(math.floor(n / 4.0 + 0.5)) - 1]
    j = np.arange(1, m + 1)
    theta = 1.0 / x[-1] + (1.0 - np.sqrt(m / (j - 0.5))) / (3.0 * x_star)
    k = np.array([np.mean(np.log1p(-th * x)) for th in theta])
    ell = n * (np.log(-theta / k) - k - 1.0)
    w = 1.0 / np.array([np.sum(np.exp(ell - e)) for e in ell])
    theta_hat = float(np.sum(theta * w))
    k_hat = float(np.mean(np.log1p(-theta_hat * x)))
    sigma = -k_hat / theta_hat
    if shrink:
        k_hat = (n * k_hat + 5.0) / (n + 10.0)
    return k_hat, sigma


def psis(v, n_keep=None, shrink=True):
    """(paretoK, elpdLoo, SNEG / den) of one star from ALL its finite values v.  n_keep: only the n_keep largest -v are
    available as a tail (what a call with that tail_len has kept); None: all of them."""
    v = np.asarray(v, dtype=np.float64)
    n_f = len(v)
    r = np.sort(-v)[::-1]                                  # descending
    rho = r - r[0]
    elpd_is = math.log(n_f) - (r[0] + math.log(np.sum(np.exp(rho))))
    M = tail_length(n_f, n_f if n_keep is None else min(n_f, n_keep))
    if M < 5:
        return np.nan, elpd_is, np.nan
    ec = math.exp(rho[M])
    x = np.sort(np.exp(rho[:M]) - ec)
    if x[-1] == 0 or not x[int(math.floor(M / 4.0 + 0.5)) - 1] > 0:
        return np.nan, elpd_is, np.nan
    k_hat, sigma = gpd_fit(x, shrink)
    p = (np.arange(1, M + 1) - 0.5) / M
    q = -sigma * np.log1p(-p) if k_hat == 0 else sigma * np.expm1(-k_hat * np.log1p(-p)) / k_hat
    w = np.minimum(1.0, ec + q)                           # of the j-th SMALLEST tail value
    rho_tail = rho[:M][::-1]                              # ascending, paired by rank
    num = (n_f - M) + np.sum(np.exp(np.log(w) - rho_tail))
    body = np.sum(np.exp(rho[M:]))                        # the non-tail sum, formed directly
    den = body + np.sum(w)
    return k_hat, math.log(num) - math.log(den) - r[0], float(np.sum(np.exp(rho))) / den


def star_row(v_all, n_keep=None, shrink=True):
    """One line of the per-star table from the star's values over the rows inside the grid (-inf allowed); also SNEG / den."""
    v_all = np.asarray(v_all, dtype=np.float64)
    rows = len(v_all)
    out = np.zeros(9)
    if rows == 0:
        return out, np.nan
    fin = v_all[np.isfinite(v_all)]
    n_f, n_inf = len(fin), rows - len(fin)
    out[T_ROWS], out[T_NINF] = rows, n_inf
    lppd = logsumexp(fin) - math.log(rows) if n_f else -np.inf
    p_waic = float(np.var(fin, ddof=1)) if n_f >= 2 else 0.0
    if n_inf > 0:
        out[T_LPPD:] = (lppd, p_waic, -np.inf, -np.inf, np.inf, -np.inf, np.inf)
        return out, np.nan
    k, loo, ratio = psis(fin, n_keep, shrink)
    elpd_is = math.log(n_f) - logsumexp(-fin)
    out[T_LPPD:] = (lppd, p_waic, lppd - p_waic, elpd_is, k, loo, lppd - loo)
    return out, ratio


def table(V, inside=None, n_keep=None, shrink=True):
    """(table [star, 9], SNEG / den [star]) from the full matrix."""
    V = np.asarray(V, dtype=np.float64)
    inside = np.ones(len(V), bool) if inside is None else inside
    got = [star_row(V[inside, i], n_keep, shrink) for i in range(V.shape[1])]
    return np.array([g[0] for g in got]).reshape(-1, 9), np.array([g[1] for g in got])


def _sum_se(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return float(np.sum(x)), (math.sqrt(len(x) * float(np.var(x, ddof=1))) if len(x) >= 2 else 0.0)


def totals(tab):
    """The totals over the stars with rows > 0, in hostlib.SCORE_TOTALS' order."""
    t = np.asarray(tab)[np.asarray(tab)[:, T_ROWS] > 0]
    k = t[:, T_K]
    fin = k[np.isfinite(k)]
    return np.array([len(t), *_sum_se(t[:, T_LPPD]), *_sum_se(t[:, T_ELPD_WAIC]), *_sum_se(t[:, T_ELPD_LOO]), np.sum(t[:, T_PWAIC]),
                     np.sum(t[:, T_PLOO]), np.sum(t[:, T_NINF] > 0), np.sum(k > 0.7), fin.max() if len(fin) else np.nan])


def compare(tab_a, tab_b):
    """(N, sum and se of elpdLoo_A - elpdLoo_B, the same for elpdWaic) over the stars with rows > 0 in both, then the number of
    stars with rows > 0 in exactly one."""
    a, b = np.asarray(tab_a), np.asarray(tab_b)
    use = (a[:, T_ROWS] > 0) & (b[:, T_ROWS] > 0)
    return np.array([use.sum(), *_sum_se(a[use, T_ELPD_LOO] - b[use, T_ELPD_LOO]), *_sum_se(a[use, T_ELPD_WAIC] - b[use, T_ELPD_WAIC]),
                     ((a[:, T_ROWS] > 0) != (b[:, T_ROWS] > 0)).sum()])
