"""numpy statement of b9_star_influence and of the starInfluence tables (tests only).  Shares no code with the kernels or the
host library: the values are pointwise_ref.v_matrix's; `accumulate` is the stated recurrence in the stated order; `direct` forms
the same sums without a recurrence, sorted, in np.longdouble; `group_sums` adds a group's stars in the caller's order; `table`
and `group_table` work on the FULL vectors (the PSIS fit through pointwise_ref.psis' pieces), not through acc / tail.

For star i, with the rows inside the grid in which v is finite, r = -v, w = exp(r - max r):  SNEG = sum w, SNEG2 = sum w^2,
WQ_j = sum w q_j, WQ2_j = sum w q_j^2, MEANV = mean v, MQ_j = mean q_j, CVQ_j = sum (v - mean v)(q_j - mean q_j).  The posterior
without star i is the chain reweighted by w, so WQ / SNEG is the mean of q without it and -CVQ / (n - 1) its first-order move."""
import math

import numpy as np

import pointwise_ref as pr

ROWS, NINF, RMAX, SNEG, SNEG2, MEANV = range(6)
HEAD = 6
STAR_HEAD = 4            # per-star table: rows, nInf, ess, paretoK, then shift, lin, looSd per quantity
GROUP_HEAD = 5           # per-group table: nStars, rows, nInf, ess, paretoK, then shiftRaw, shift, looSd per quantity
MUTANTS = ("wq2_not_rescaled", "sneg2_f", "cvq_old_mean", "inf_counts_in_k", "k_for_k1")


def WQ(j):
    return 6 + 4 * j


def N(n_q):
    return 6 + 4 * n_q


# ---- the recurrence ---------------------------------------------------------------------------------------------------------
def accumulate(V, inside, q, acc=None, mutant=None):
    """acc [star, 6 + 4 Q] after the rows of V in ascending order.  mutant: one of MUTANTS, the faults the comparators must
    reject (WQ2 not rescaled at a jump; f for f f in SNEG2; the old mean in CVQ; -inf rows counted in k; k for k + 1)."""
    assert mutant is None or mutant in MUTANTS
    V = np.asarray(V, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64).reshape(len(V), -1)
    n_rows, n = V.shape
    Q = q.shape[1]
    inside = np.ones(n_rows, bool) if inside is None else inside
    acc = np.zeros((n, N(Q))) if acc is None else np.array(acc, dtype=np.float64).reshape(n, N(Q))
    fma = getattr(math, "fma", None) or (lambda a, b, c: float(np.longdouble(a) * np.longdouble(b) + np.longdouble(c)))
    for r in range(n_rows):
        if not inside[r]:
            continue
        for i in range(n):
            a, v = acc[i], float(V[r, i])
            k = a[ROWS] if mutant == "inf_counts_in_k" else a[ROWS] - a[NINF]
            a[ROWS] += 1.0
            if v == -np.inf:
                a[NINF] += 1.0
                continue
            x = -v
            if k == 0:
                a[RMAX:HEAD] = (x, 1.0, 1.0, v)
                for j in range(Q):
                    y = float(q[r, j])
                    a[WQ(j):WQ(j) + 4] = (y, y * y, y, 0.0)
                continue
            if x > a[RMAX]:
                f = math.exp(a[RMAX] - x)
                ff = f if mutant == "sneg2_f" else f * f
                a[SNEG] = fma(a[SNEG], f, 1.0)
                a[SNEG2] = fma(a[SNEG2], ff, 1.0)
                for j in range(Q):
                    y = float(q[r, j])
                    a[WQ(j)] = fma(a[WQ(j)], f, y)
                    a[WQ(j) + 1] = fma(a[WQ(j) + 1], 1.0 if mutant == "wq2_not_rescaled" else f, y * y)
                a[RMAX] = x
            else:
                e = math.exp(x - a[RMAX])
                a[SNEG] = a[SNEG] + e
                a[SNEG2] = fma(e, e, a[SNEG2])
                for j in range(Q):
                    y = float(q[r, j])
                    a[WQ(j)] = fma(e, y, a[WQ(j)])
                    a[WQ(j) + 1] = fma(e * y, y, a[WQ(j) + 1])
            div = k if mutant == "k_for_k1" else k + 1.0
            dv = v - a[MEANV]
            a[MEANV] += dv / div
            for j in range(Q):
                y = float(q[r, j])
                old = a[WQ(j) + 2]
                a[WQ(j) + 2] += (y - old) / div
                a[WQ(j) + 3] = fma(dv, y - (old if mutant == "cvq_old_mean" else a[WQ(j) + 2]), a[WQ(j) + 3])
    return acc


# ---- the same sums, formed directly -----------------------------------------------------------------------------------------
def _sorted_sum(t):
    """sum of t in np.longdouble, the terms taken in ascending magnitude"""
    t = np.asarray(t, dtype=np.longdouble)
    return np.sum(t[np.argsort(np.abs(t), kind="stable")], dtype=np.longdouble) if len(t) else np.longdouble(0)


def direct(V, inside, q):
    """(acc [star, 6 + 4 Q] in float64 from long-double sorted sums, abs [star, 2 + 3 Q]: the sums of the terms' magnitudes --
    sum w, sum |v - mean v|, then per quantity sum w |q|, sum w q^2, sum |v - mean v| |q - mean q| -- which the bounds of
    influence_check are stated on)."""
    V = np.asarray(V, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64).reshape(len(V), -1)
    inside = np.ones(len(V), bool) if inside is None else np.asarray(inside, bool)
    n, Q = V.shape[1], q.shape[1]
    acc, mag = np.zeros((n, N(Q))), np.zeros((n, 2 + 3 * Q))
    for i in range(n):
        v = V[inside, i]
        fin = np.isfinite(v)
        acc[i, ROWS], acc[i, NINF] = len(v), len(v) - fin.sum()
        if not fin.any():
            continue
        vl, ql = v[fin].astype(np.longdouble), q[inside][fin].astype(np.longdouble)
        rmax = np.max(-vl)
        w = np.exp(-vl - rmax)
        mv = _sorted_sum(vl) / len(vl)
        acc[i, RMAX:HEAD] = (rmax, _sorted_sum(w), _sorted_sum(w * w), mv)
        mag[i, :2] = (_sorted_sum(w), _sorted_sum(np.abs(vl - mv)))
        for j in range(Q):
            y = ql[:, j]
            my = _sorted_sum(y) / len(y)
            acc[i, WQ(j):WQ(j) + 4] = (_sorted_sum(w * y), _sorted_sum(w * y * y), my, _sorted_sum((vl - mv) * (y - my)))
            mag[i, 2 + 3 * j:5 + 3 * j] = (_sorted_sum(w * np.abs(y)), _sorted_sum(w * y * y), _sorted_sum(np.abs(vl - mv) * np.abs(y - my)))
    return acc, mag


def group_sums(V, inside, group, n_groups, ignore_ids=False):
    """group_lpd [row, group]: the stars of a group added in ascending order from +0.0, one add each; -inf for a row outside the
    grid.  ignore_ids: every star taken into every group, a MUTATION."""
    V = np.asarray(V, dtype=np.float64)
    out = np.full((len(V), n_groups), -np.inf)
    for r in np.flatnonzero(inside):
        for g in range(n_groups):
            a = 0.0
            for i, x in enumerate(V[r]):
                if ignore_ids or group[i] == g:
                    a = a + float(x)
            out[r, g] = a
    return out


# ---- the tables, on the full vectors ----------------------------------------------------------------------------------------
def _moments(w, y):
    sw = np.sum(w)
    m = np.sum(w * y) / sw
    return m, math.sqrt(max(0.0, float(np.sum(w * y * y) / sw - m * m)))


def star_row(v_all, q_all, n_keep=None, sign_shift=1.0, sign_lin=-1.0, ess_plain=False):
    """One line of the per-star table from the star's values and the quantities over the rows inside the grid.  sign_shift = -1,
    sign_lin = +1 and ess_plain (SNEG / SNEG2): three MUTATIONS."""
    v_all = np.asarray(v_all, dtype=np.float64)
    q_all = np.asarray(q_all, dtype=np.float64).reshape(len(v_all), -1)
    Q = q_all.shape[1]
    out = np.zeros(STAR_HEAD + 3 * Q)
    if len(v_all) == 0:
        return out
    fin = np.isfinite(v_all)
    out[0], out[1] = len(v_all), len(v_all) - fin.sum()
    if out[1] > 0:
        out[2:] = np.nan
        out[2] = 0.0
        return out
    v, q = v_all, q_all
    w = np.exp(-v - np.max(-v))
    out[2] = np.sum(w) / np.sum(w * w) if ess_plain else np.sum(w) ** 2 / np.sum(w * w)
    out[3] = pr.psis(v, n_keep)[0]
    for j in range(Q):
        m, sd = _moments(w, q[:, j])
        lin = sign_lin * float(np.sum((v - v.mean()) * (q[:, j] - q[:, j].mean()))) / (len(v) - 1) if len(v) >= 2 else 0.0
        out[STAR_HEAD + 3 * j:STAR_HEAD + 3 * j + 3] = (sign_shift * (m - q[:, j].mean()), lin, sd)
    return out


def table(V, inside, q, n_keep=None, **mutation):
    V = np.asarray(V, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64).reshape(len(V), -1)
    inside = np.ones(len(V), bool) if inside is None else np.asarray(inside, bool)
    return np.array([star_row(V[inside, i], q[inside], n_keep, **mutation) for i in range(V.shape[1])]).reshape(V.shape[1], -1)


def smoothed_weights(rho):
    """(paretoK, w [row]) of the full vector rho (finite): w = e^(rho - max rho) with the M largest replaced by the smoothed
    weights of steps (1) - (6), paired by rank (ties in rho: the earlier row ranks higher); (NaN, the raw weights) where the fit is
    refused."""
    rho = np.asarray(rho, dtype=np.float64)
    n_f = len(rho)
    order = np.argsort(-rho, kind="stable")              # descending
    d = rho[order] - rho[order[0]]
    w = np.exp(rho - rho[order[0]])
    M = pr.tail_length(n_f, n_f)
    if M < 5:
        return np.nan, w
    ec = math.exp(d[M])
    x = np.sort(np.exp(d[:M]) - ec)
    if x[-1] == 0 or not x[int(math.floor(M / 4.0 + 0.5)) - 1] > 0:
        return np.nan, w
    k_hat, sigma = pr.gpd_fit(x)
    p = (np.arange(1, M + 1) - 0.5) / M
    qq = -sigma * np.log1p(-p) if k_hat == 0 else sigma * np.expm1(-k_hat * np.log1p(-p)) / k_hat
    w = w.copy()
    w[order[:M][::-1]] = np.minimum(1.0, ec + qq)          # the j-th SMALLEST tail value takes the j-th quantile
    return k_hat, w


def group_table(group_lpd, q, group, **mutation):
    """[group, 5 + 3 Q] from group_lpd [row, group], q [row, Q] and the stars' ids."""
    L = np.asarray(group_lpd, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64).reshape(len(L), -1)
    G, Q = L.shape[1], q.shape[1]
    out = np.zeros((G, GROUP_HEAD + 3 * Q))
    sign = mutation.get("sign_shift", 1.0)
    for g in range(G):
        t = out[g]
        t[0] = np.sum(np.asarray(group) == g)
        fin = np.isfinite(L[:, g])
        t[1], t[2] = len(L), len(L) - fin.sum()
        if len(L) == 0:
            continue
        if t[2] > 0:
            t[3] = 0.0
            t[4:] = np.nan
            continue
        rho = -L[:, g]
        raw = np.exp(rho - rho.max())
        t[3] = np.sum(raw) / np.sum(raw * raw) if mutation.get("ess_plain") else np.sum(raw) ** 2 / np.sum(raw * raw)
        t[4], w = smoothed_weights(rho)
        for j in range(Q):
            m_raw, _ = _moments(raw, q[:, j])
            m, sd = _moments(w, q[:, j])
            t[GROUP_HEAD + 3 * j:GROUP_HEAD + 3 * j + 3] = (sign * (m_raw - q[:, j].mean()), sign * (m - q[:, j].mean()), sd)
    return out


def zscores(theta):
    """((theta - mean) / sd [row, Q], mean [Q], sd [Q]): two-pass mean, ddof-1 sd, over the rows."""
    theta = np.asarray(theta, dtype=np.float64).reshape(len(theta), -1)
    mean = theta.mean(axis=0)
    sd = np.sqrt(((theta - mean) ** 2).sum(axis=0) / (len(theta) - 1))
    return (theta - mean) / sd, mean, sd
