"""Statistical checkers for the library's random outputs (tests only), and the problems they are run on.

The draws of b9_sample_mass / b9_sample_wd_mass and the Metropolis chain are compared here with distributions that are
stated independently of the sampler's design: the numpy posterior over the grid (tests/numpy_ref.py: marg_terms,
marg_terms_wd), analytic targets (uniform, normal, truncated normal) and a brute-force one-dimensional posterior on a grid.
Nothing here calls the C oracle or a kernel: the caller hands in the draws.

Every checker prints the figure it judges, asserts its own power condition (enough nodes with an expected count, a small
enough standard error) and returns the figure; the caller asserts the threshold (P_MIN, Z_MAX), so that the mutation tests
can assert the opposite on a deliberately wrong reference.
"""
import functools

import numpy as np
from scipy import stats
from scipy.special import logsumexp

import numpy_ref
from base_amd import abi, mcmc, synth
from conftest import build_problem

_trapz = getattr(np, "trapezoid", None) or np.trapz

P_MIN, Z_MAX = 1e-4, 5.0                 # a check passes at p > P_MIN, |z| <= Z_MAX
P_REJECT, Z_REJECT = 1e-6, 8.0           # a mutated reference must be rejected at p < P_REJECT or |z| > Z_REJECT
MIN_EXPECT, MIN_NODES = 5.0, 8           # chi-square cells: expected count >= 5; a posterior must fill >= 8 of them

# seeds: constants, written down before the first run
SEED_CATALOGUE, SEED_DRAW, SEED_COPIES, SEED_WD = 31, 20250311, 20250312, 20250313
SEED_CHAIN_A, SEED_CHAIN_B, SEED_START = 20250314, 20250315, 7


# ---- the chi-square family ------------------------------------------------------------------------------------------------
def posterior(terms):
    """Probabilities of the nodes from their log-terms (-inf / NaN: a node that cannot be drawn)."""
    t = np.where(np.isfinite(terms), terms, -np.inf)
    return np.exp(t - logsumexp(t))


def pooled(count, expect, min_expect=MIN_EXPECT):
    """Cells with expected count >= min_expect kept, the others pooled into one: (count, expect, number kept)."""
    big = expect >= min_expect
    c, e = list(count[big]), list(expect[big])
    if (~big).any() and expect[~big].sum() > 0:
        c.append(count[~big].sum()); e.append(expect[~big].sum())
    return np.array(c, float), np.array(e, float), int(big.sum())


def gof(label, idx, prob, min_nodes=MIN_NODES):
    """Chi-square goodness of fit of the drawn node indices against prob.  A draw on a node of probability 0 fails outright.
    Power condition (asserted): at least min_nodes nodes with expected count >= 5.  Returns p."""
    idx = np.asarray(idx).ravel()
    count = np.bincount(idx, minlength=len(prob)).astype(float)
    assert np.all(count[prob == 0] == 0), f"{label}: a draw on a node of probability 0"
    c, e, n_big = pooled(count, prob * len(idx))
    chi2 = float(np.sum((c - e) ** 2 / e))
    dof = len(c) - 1
    p = float(stats.chi2.sf(chi2, dof))
    print(f"{label}: goodness of fit chi2 {chi2:.2f}, {dof} dof, p {p:.3g}; {n_big} nodes with expected count >= 5, {len(idx)} draws")
    assert n_big >= min_nodes, f"{label}: the posterior sits on {n_big} nodes, too few for the test to say anything"
    return p


def independence(label, a, idx, n_nodes, min_nodes=MIN_NODES):
    """Chi-square test of independence of a two-valued draw a and the node index idx.  Nodes whose smaller expected cell is
    below 5 are pooled.  Power condition (asserted): at least min_nodes columns kept.  Returns p."""
    a, idx = np.asarray(a).ravel(), np.asarray(idx).ravel()
    table = np.stack([np.bincount(idx[a == v], minlength=n_nodes) for v in (0, 1)]).astype(float)
    rows, cols, n = table.sum(axis=1), table.sum(axis=0), table.sum()
    small = np.outer(rows, cols).min(axis=0) / n < MIN_EXPECT
    t = np.concatenate([table[:, ~small], table[:, small].sum(axis=1, keepdims=True)], axis=1) if small.any() else table
    t = t[:, t.sum(axis=0) > 0]
    chi2, p, dof, _ = stats.chi2_contingency(t, correction=False)
    print(f"{label}: independence chi2 {chi2:.2f}, {dof} dof, p {p:.3g}; {int((~small).sum())} nodes kept, {int(n)} draws")
    assert int((~small).sum()) >= min_nodes, f"{label}: too few nodes with both expected cells >= 5"
    return float(p)


def binomial_z(label, k, n, p):
    """z of a count k of n against the binomial (n, p).  Power condition (asserted): n p (1 - p) >= 25."""
    assert n * p * (1 - p) >= 25, f"{label}: too few draws for the normal approximation"
    z = float((k - n * p) / np.sqrt(n * p * (1 - p)))
    print(f"{label}: {k} of {n}, expected {n * p:.1f}, z {z:+.2f}")
    return z


def coincidence_z(label, a, b, prob, linked=0):
    """Two independent draws from prob fall on the same node with probability c = sum p^2.  a, b: node indices, pair k being
    (a[k], b[k]).  z of the number of coincidences against n c.  Pairs that share a draw (copy i with i + 1 and i + 1 with
    i + 2) are not independent of each other: `linked` is the number of such couples of pairs, each adding
    2 (sum p^3 - c^2) to the variance n c (1 - c).  Power condition (asserted): >= 50 coincidences expected, c <= 1/2 --
    an aliased counter (every pair equal) then stands at z of order sqrt(n)."""
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    n, c = len(a), float(np.sum(prob ** 2))
    var = n * c * (1 - c) + 2 * linked * (float(np.sum(prob ** 3)) - c * c)
    k = int(np.sum(a == b))
    assert n * c >= 50 and c <= 0.5, f"{label}: c = {c:.3g} over {n} pairs gives the test no power"
    z = float((k - n * c) / np.sqrt(var))
    print(f"{label}: {k} coincidences in {n} pairs, expected {n * c:.1f} (c = {c:.4f}), z {z:+.2f}")
    return z


def worst_pair_z(label, a, b, prob):
    """The coincidence z of every column pair (a[:, k], b[:, k]) on its own, rows being independent: the largest in absolute
    value.  The pooled count would dilute one aliased pair of copies among a hundred; this does not.  Power condition
    (asserted): >= 20 coincidences expected per pair (the normal approximation), and a pair that always coincides, at
    z = sqrt(n (1 - c) / c), stands at ten times Z_MAX or more."""
    n, c = a.shape[0], float(np.sum(prob ** 2))
    assert n * c >= 20 and np.sqrt(n * (1 - c) / c) >= 10 * Z_MAX, f"{label}: c = {c:.3g} over {n} rows gives the test no power"
    z = ((a == b).sum(axis=0) - n * c) / np.sqrt(n * c * (1 - c))
    k = int(np.argmax(np.abs(z)))
    print(f"{label}: worst of {len(z)} pairs is pair {k}, z {z[k]:+.2f}")
    return float(z[k])


def neighbour_checks(label, idx, prob):
    """idx[row, copy]: the coincidence test between neighbouring copies, copies 64 apart and neighbouring rows.
    Returns {name: z}."""
    R, n = idx.shape
    out = {"copies i, i+1": coincidence_z(f"{label}, copies (i, i+1)", idx[:, :-1], idx[:, 1:], prob, linked=R * (n - 2))}
    if n > 64:
        out["copies i, i+64"] = coincidence_z(f"{label}, copies (i, i+64)", idx[:, :-64], idx[:, 64:], prob, linked=R * max(0, n - 128))
    out["worst pair i, i+1"] = worst_pair_z(f"{label}, copies (i, i+1) one pair at a time", idx[:, :-1], idx[:, 1:], prob)
    if n > 64:
        out["worst pair i, i+64"] = worst_pair_z(f"{label}, copies (i, i+64) one pair at a time", idx[:, :-64], idx[:, 64:], prob)
    out["rows r, r+1"] = coincidence_z(f"{label}, rows (r, r+1)", idx[:-1], idx[1:], prob, linked=(R - 2) * n)
    return out


# ---- draws back to nodes ---------------------------------------------------------------------------------------------------
def node_index(mass, ratio, g_mass, g_ratio):
    """The index of every draw (mass, ratio) in the grid of numpy_ref.marg_terms (ratio-major) or marg_terms_wd (ratio 0);
    every draw must be a node to 1e-12 relative."""
    mass, ratio = np.asarray(mass, float), np.asarray(ratio, float)
    levels = np.unique(g_ratio)
    Q, P = len(levels), len(g_mass) // len(levels)
    mp = g_mass[:P]
    assert np.all(np.diff(mp) > 0) and np.array_equal(g_mass, np.tile(mp, Q))
    j = np.rint(ratio * Q).astype(int)
    assert np.all((j >= 0) & (j < Q)) and np.all(np.abs(ratio - j / Q) <= 1e-12), "a drawn mass ratio is no grid value"
    k = np.clip(np.searchsorted(mp, mass), 1, P - 1)
    k = np.where(np.abs(mp[k - 1] - mass) < np.abs(mp[k] - mass), k - 1, k)
    assert np.all(np.abs(mp[k] - mass) <= 1e-12 * np.abs(mp[k])), "a drawn mass is no grid node"
    return j * P + k


# ---- the Metropolis chain --------------------------------------------------------------------------------------------------
BATCH = 500                               # batch means: at least 500 consecutive steps of one walker
SE_MEAN_MAX, SE_VAR_MAX = 0.03, 0.06      # power: se of a mean <= 0.03 target sd, relative se of a variance <= 0.06


def _batch_se(v, batch):
    """Standard error of the mean of v[step, walker] from the means of batches of consecutive steps of one walker."""
    nb = v.shape[0] // batch
    assert batch >= BATCH and nb * v.shape[1] >= 20, "too few batches for a standard error"
    bm = v[:nb * batch].reshape(nb, batch, v.shape[1]).mean(axis=1).ravel()
    return float(bm.std(ddof=1) / np.sqrt(len(bm)))


def moments(label, x, mean0, var0, batch=BATCH):
    """z of the pooled mean and variance of the chain x[step, walker] against the target's mean0, var0, on batch-means
    standard errors.  Power condition (asserted): se(mean) <= 0.03 sd0 and se(var) <= 0.06 var0.  Returns (z_mean, z_var)."""
    m = float(x.mean())
    d2 = (x - m) ** 2
    v = float(d2.mean())
    se_m, se_v = _batch_se(x, batch), _batch_se(d2, batch)
    zm, zv = (m - mean0) / se_m, (v - var0) / se_v
    print(f"{label}: mean {m:.6g} (target {mean0:.6g}, se {se_m / np.sqrt(var0):.4f} sd, z {zm:+.2f}); "
          f"variance {v:.6g} (target {var0:.6g}, relative se {se_v / var0:.4f}, z {zv:+.2f})")
    assert se_m <= SE_MEAN_MAX * np.sqrt(var0), f"{label}: se of the mean {se_m / np.sqrt(var0):.4f} sd: too few steps"
    assert se_v <= SE_VAR_MAX * var0, f"{label}: relative se of the variance {se_v / var0:.4f}: too few steps"
    return float(zm), float(zv)


def correlation_z(label, x, y, batch=BATCH):
    """z of the chain's correlation of x and y against 0, on a batch-means standard error (asserted <= 0.03)."""
    u = (x - x.mean()) * (y - y.mean()) / (x.std() * y.std())
    r, se = float(u.mean()), _batch_se(u, batch)
    print(f"{label}: correlation {r:+.4f}, se {se:.4f}, z {r / se:+.2f}")
    assert se <= SE_MEAN_MAX, f"{label}: se of the correlation {se:.4f}: too few steps"
    return r / se


def run_chain(runner, evaluate, start, free, steps, n_burn, n_keep, seed, block=100, keep_block=2000):
    """WalkerSampler: a burn-in with adaptation, then n_keep steps with the proposal frozen; only those are returned,
    [step, walker, d], with the acceptance rate of the frozen part."""
    s = mcmc.WalkerSampler(start, runner, free=free, seed=seed, block=block, step_sizes=dict(zip(free, steps)))
    s.initialise(evaluate)
    s.run(n_burn)
    s.block, acc0, rec = keep_block, s.accepted, []
    s.run(n_keep, rec, adapt=False)
    return np.concatenate([r[0] for r in rec]), (s.accepted - acc0) / (n_keep * len(start))


# ---- problems: b9_sample_mass --------------------------------------------------------------------------------------------
PER_STAR = ("obs", "sigma", "mass1", "mass_ratio", "clust_prior", "stage", "wd_type", "is_field", "pop")
K_MASS, Q_MASS, R_MASS, R_COPIES, N_COPIES = 2, 3, 4000, 500, 130
LAMBDA = 0.35


def subset(cl, sel):
    out = dict(cl)
    for k in PER_STAR:
        out[k] = np.ascontiguousarray(np.asarray(cl[k])[sel])
    return out


def star_terms(pack_d, cl, par, n_pops, K=K_MASS, Q=Q_MASS, wd_nodes=None):
    """Per population: (terms[star, node] padded with -inf, [grid of MS/RGB stars, grid of WD-stage stars]).  A WD-stage
    star's row holds its WD-node terms (its own atmosphere type), any other star's the (mass, ratio) grid's."""
    wd = np.asarray(cl["stage"]) == abi.STAGE_WD
    out = []
    for pop in range(n_pops):
        t, gm, gq = numpy_ref.marg_terms(pack_d, cl, par, K, Q, pop)
        tw, gw = numpy_ref.marg_terms_wd(pack_d, cl, par, K, pop, n_nodes=wd_nodes) if wd.any() else (None, None)
        rows = []
        for i in range(len(wd)):
            r = np.full(max(t.shape[1], 0 if tw is None else tw.shape[1]), -np.inf)
            src = tw[i] if wd[i] else t[i]
            r[:len(src)] = np.where(np.isfinite(src), src, -np.inf)
            rows.append(r)
        out.append((np.array(rows), (gm, gq), (gw, None if gw is None else np.zeros(len(gw)))))
    return out


def joint_posterior(terms_by_pop, i, lam):
    """Star i's probabilities over (population, node), population-major, and log L of each population."""
    if len(terms_by_pop) == 1:
        return posterior(terms_by_pop[0][0][i]), [logsumexp(terms_by_pop[0][0][i])]
    with np.errstate(divide="ignore"):
        t = np.concatenate([np.log(lam) + terms_by_pop[0][0][i], np.log1p(-lam) + terms_by_pop[1][0][i]])
    return posterior(t), [logsumexp(terms_by_pop[0][0][i]), logsumexp(terms_by_pop[1][0][i])]


def draws_to_index(terms_by_pop, cl, i, mass, ratio, pop):
    """Joint (population, node) index of star i's draws."""
    wd = np.asarray(cl["stage"])[i] == abi.STAGE_WD
    width = terms_by_pop[0][0].shape[1]
    idx = np.empty(len(mass), int)
    for k in range(len(terms_by_pop)):
        sel = pop == k
        if sel.any():
            g = terms_by_pop[k][2] if wd else terms_by_pop[k][1]
            idx[sel] = k * width + node_index(mass[sel], ratio[sel], g[0], g[1])
    return idx


def filled_nodes(prob, n_draws, n_pops):
    """Nodes with expected count >= 5 in n_draws draws from the joint (population, node) table prob: the smaller of the
    populations' counts, so that each population's half of the table can be tested on its own."""
    return min(int(np.sum(half * n_draws >= MIN_EXPECT)) for half in np.split(prob, n_pops))


@functools.lru_cache(maxsize=None)
def mass_problem(n_pops=1, same_y=False):
    """About 8 stars on a short isochrone: five main-sequence singles, a binary with mass ratio > 0.5, a DA and a DB WD-stage
    star.  Each star's photometric sigmas are widened (x 1.5 at a time, judged on the numpy posterior alone) until its
    posterior has at least MIN_NODES nodes with expected count >= 5 in R_MASS draws (two populations: in each population's
    half of the joint table)."""
    pack_d, cl, _, _, priors, _ = build_problem("parsec", 5, n_stars=80, wd_frac=0.15, n_y=3 if n_pops == 2 else 1, n_pops=n_pops,
                                                seed=SEED_CATALOGUE, n_feh=3, n_age=4, n_eep=25)
    stage, q, field = np.asarray(cl["stage"]), np.asarray(cl["mass_ratio"]), np.asarray(cl["is_field"])
    ms = np.flatnonzero((stage != abi.STAGE_WD) & (q == 0) & ~field)[:5]
    binary = np.flatnonzero((stage != abi.STAGE_WD) & (q > 0.5) & ~field)[:1]
    wds = np.flatnonzero((stage == abi.STAGE_WD) & ~field)[:2]
    assert len(ms) == 5 and len(binary) == 1 and len(wds) == 2
    cl = subset(cl, np.concatenate([ms, binary, wds]))
    cl["wd_type"][6], cl["wd_type"][7] = 0, 1                                   # one DA, one DB
    cl["sigma"] = np.where(cl["sigma"] > 0, cl["sigma"] * 3.0, cl["sigma"])
    par = np.array(cl["truth"], dtype=np.float64)
    if n_pops == 2:
        par[abi.P_LAMBDA] = 0.5 if same_y else LAMBDA
        if same_y:
            par[abi.P_Y2] = par[abi.P_Y]
    for _ in range(40):
        tb = star_terms(pack_d, cl, par, n_pops)
        thin = [i for i in range(8) if filled_nodes(joint_posterior(tb, i, par[abi.P_LAMBDA])[0], R_MASS, n_pops) < MIN_NODES]
        if not thin:
            break
        cl["sigma"][thin] = np.where(cl["sigma"][thin] > 0, cl["sigma"][thin] * 1.5, cl["sigma"][thin])
    return pack_d, cl, priors, par, tb


def copies_problem(n_pops=1):
    """Star 0 of mass_problem copied N_COPIES times: more than two waves of one workgroup, across the 64- and 128-lane edges.
    Two populations: Y2 = Y and lambda = 0.5, so that the population is a fair coin independent of the node."""
    pack_d, cl, priors, par, tb = mass_problem(n_pops, same_y=True)
    return pack_d, subset(cl, np.zeros(N_COPIES, int)), priors, par, [(t[0][:1], t[1], t[2]) for t in tb]


def member_from(cl, i, logL, lam):
    """The membership probability the numpy marginals imply."""
    log_fs = -np.sum(np.log(cl["filter_prior_max"] - cl["filter_prior_min"]))
    pm = np.asarray(cl["clust_prior"])[i]
    L = logL[0] if len(logL) == 1 else np.logaddexp(np.log(lam) + logL[0], np.log1p(-lam) + logL[1])
    return float(np.clip(np.exp(np.log(pm) + L - np.logaddexp(np.log1p(-pm) + log_fs, np.log(pm) + L)), 0, 1))


def check_mass_posterior(draw, n_pops=1, same_y=False):
    """Part 1 of the draws' tests on `draw(pack_d, cl, priors, n_pops, K, Q, rows, seed, row0) -> (mass, ratio, member, pop)`:
    per star the goodness of fit of its R_MASS draws against the numpy posterior over (population, node), the membership,
    the population count, and for Y2 = Y the conditional node distributions.  Returns {label: figure} after asserting."""
    pack_d, cl, priors, par, tb = mass_problem(n_pops, same_y)
    lam = par[abi.P_LAMBDA]
    mass, ratio, member, pop = draw(pack_d, cl, priors, n_pops, K_MASS, Q_MASS, np.repeat(par[None], R_MASS, axis=0), SEED_DRAW, 0)
    wd = np.asarray(cl["stage"]) == abi.STAGE_WD
    width = tb[0][0].shape[1]
    fig = {}
    for i in range(len(wd)):
        kind = "WD-stage" if wd[i] else ("binary" if cl["mass_ratio"][i] > 0 else "single")
        label = f"star {i} ({kind}, {n_pops} pop)"
        prob, logL = joint_posterior(tb, i, lam)
        if wd[i]:
            assert np.all(ratio[:, i] == 0), "a WD-stage star drew a companion"
        if n_pops == 1:
            assert np.all(pop[:, i] == 0)
        idx = draws_to_index(tb, cl, i, mass[:, i], ratio[:, i], pop[:, i])
        assert filled_nodes(prob, R_MASS, n_pops) >= MIN_NODES, f"{label}: the posterior sits on too few nodes"
        fig[f"{label} p"] = p = gof(label, idx, prob)
        assert p > P_MIN, label
        np.testing.assert_allclose(member[:, i], member_from(cl, i, logL, lam), rtol=1e-9, atol=1e-12)
        if n_pops == 2:
            p_a = float(np.exp(np.log(lam) + logL[0] - np.logaddexp(np.log(lam) + logL[0], np.log1p(-lam) + logL[1])))
            if same_y:
                assert abs(p_a - 0.5) < 1e-12
            fig[f"{label} z(pop)"] = z = binomial_z(f"{label}, population A at p_A = {p_a:.4f}", int(np.sum(pop[:, i] == 0)), R_MASS, p_a)
            assert abs(z) <= Z_MAX, label
            if same_y:                                                  # given the population, the one-population posterior
                cond = posterior(tb[0][0][i])
                for k in (0, 1):
                    fig[f"{label} p(node | pop {k})"] = p = gof(f"{label}, given population {k}", idx[pop[:, i] == k] - k * width, cond, min_nodes=MIN_NODES - 1)
                    assert p > P_MIN, label
    return fig


def check_copies(draw, n_pops=1):
    """Part 2: N_COPIES copies of one star, R_COPIES equal rows.  Pooled goodness of fit; coincidences between neighbouring
    copies, copies 64 apart and neighbouring rows; for two populations the independence of population and node and the
    coincidences between the draws that fell to A and those that fell to B.  Returns (figures, idx, pop, prob)."""
    pack_d, cl, priors, par, tb = copies_problem(n_pops)
    mass, ratio, member, pop = draw(pack_d, cl, priors, n_pops, K_MASS, Q_MASS, np.repeat(par[None], R_COPIES, axis=0), SEED_COPIES, 0)
    prob, _ = joint_posterior(tb, 0, par[abi.P_LAMBDA])
    idx = np.stack([draws_to_index(tb, cl, 0, mass[:, c], ratio[:, c], pop[:, c]) for c in range(N_COPIES)], axis=1)
    label = f"{N_COPIES} copies x {R_COPIES} rows ({n_pops} pop)"
    fig = {"pooled p": gof(label, idx, prob)}
    assert fig["pooled p"] > P_MIN
    for name, z in neighbour_checks(label, idx, prob).items():
        fig[f"z {name}"] = z
        assert abs(z) <= Z_MAX, name
    if n_pops == 2:
        width = tb[0][0].shape[1]
        node = idx % width
        fig["p independence"] = p = independence(label, pop, node, width)
        assert p > P_MIN
        # the draws that fell to A against those that fell to B, paired in order of appearance: the nodes of two different
        # draws, one per population, coincide with probability sum p_node^2
        a, b = node[pop == 0], node[pop == 1]
        n = min(len(a), len(b))
        fig["z A against B"] = z = coincidence_z(f"{label}, population A against B", a[:n], b[:n], posterior(tb[0][0][0]))
        assert abs(z) <= Z_MAX
    return fig, idx, pop, prob


# ---- problems: b9_sample_wd_mass -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wd_copies_problem(n_nodes):
    """N_COPIES copies of one WD-stage star, two populations (Y2 != Y: two grids), lambda = LAMBDA."""
    pack_d, cl, _, _, priors, _ = build_problem("parsec", 5, n_stars=80, wd_frac=0.15, n_y=3, n_pops=2, seed=SEED_CATALOGUE,
                                                n_feh=3, n_age=4, n_eep=25)
    wd = np.flatnonzero((np.asarray(cl["stage"]) == abi.STAGE_WD) & ~np.asarray(cl["is_field"]))[:1]
    cl = subset(cl, np.repeat(wd, N_COPIES))
    cl["sigma"] = np.where(cl["sigma"] > 0, cl["sigma"] * 3.0, cl["sigma"])
    par = np.array(cl["truth"], dtype=np.float64)
    par[abi.P_LAMBDA] = LAMBDA
    one = subset(cl, np.zeros(1, int))
    tb = []
    for pop in (0, 1):
        t, g = numpy_ref.marg_terms_wd(pack_d, one, par, 1, pop, n_nodes=n_nodes)
        tb.append((np.where(np.isfinite(t), t, -np.inf), None, (g, np.zeros(len(g)))))
    return pack_d, cl, priors, par, tb


def check_wd_copies(draw_wd, n_nodes):
    """`draw_wd(pack_d, cl, priors, rows, n_nodes, seed) -> (zams, pop)`: the checks of check_copies on the WD sampler's
    joint (population, node) draw."""
    pack_d, cl, priors, par, tb = wd_copies_problem(n_nodes)
    zams, pop = draw_wd(pack_d, cl, priors, np.repeat(par[None], R_COPIES, axis=0), n_nodes, SEED_WD)
    prob, logL = joint_posterior(tb, 0, par[abi.P_LAMBDA])
    idx = np.stack([draws_to_index(tb, cl, 0, zams[:, c], np.zeros(R_COPIES), pop[:, c]) for c in range(N_COPIES)], axis=1)
    label = f"WD sampler, {N_COPIES} copies x {R_COPIES} rows, {n_nodes} nodes, 2 pop"
    fig = {"pooled p": gof(label, idx, prob)}
    assert fig["pooled p"] > P_MIN
    lam = par[abi.P_LAMBDA]
    p_a = float(np.exp(np.log(lam) + logL[0] - np.logaddexp(np.log(lam) + logL[0], np.log1p(-lam) + logL[1])))
    fig["z(pop)"] = z = binomial_z(f"{label}, population A at p_A = {p_a:.4f}", int(np.sum(pop == 0)), pop.size, p_a)
    assert abs(z) <= Z_MAX
    for name, z in neighbour_checks(label, idx, prob).items():
        fig[f"z {name}"] = z
        assert abs(z) <= Z_MAX, name
    return fig


# ---- problems: the chain, target A (constant likelihood: the prior is the posterior) -----------------------------------------
A_AGE = (9.25, 9.35)                      # log-age window, strictly inside the grid: uniform with two hard walls
A_SD = {abi.P_FEH: 0.05, abi.P_MOD: 0.05, abi.P_ABS: 0.05}     # grid edges of [Fe/H] (-2, 0.5) are >= 13 sd from -0.15
A_ABS_MEAN = 0.025                        # 0.5 sd: the wall abs >= 0 cuts the bulk


@functools.lru_cache(maxsize=None)
def target_a_problem(marginalised=False):
    pack_d, cl, _, _, priors, _ = build_problem("parsec", 5, n_stars=64, wd_frac=0.05, seed=SEED_CATALOGUE, n_feh=3, n_age=4, n_eep=25)
    cl["clust_prior"] = np.full(64, 1e-300)
    truth = np.array(cl["truth"], dtype=np.float64)
    mean, var = truth.copy(), np.zeros(abi.B9_NPARAM)
    mean[abi.P_ABS] = A_ABS_MEAN
    for k, sd in A_SD.items():
        var[k] = sd * sd
    priors = abi.make_priors(mean, var, *A_AGE)
    assert pack_d["log_age"][0] < A_AGE[0] and A_AGE[1] < pack_d["log_age"][-1]
    assert min(mean[abi.P_FEH] - pack_d["feh"][0], pack_d["feh"][-1] - mean[abi.P_FEH]) >= 8 * A_SD[abi.P_FEH]
    opt = (abi.MODE_MARGINALISED, 1, 1, 1) if marginalised else (abi.MODE_GIVEN_MASS, 1, 4, 4)
    return pack_d, cl, priors, mean, opt


def target_a_moments():
    """{parameter: (mean, variance)} of target A."""
    tn = stats.truncnorm(-A_ABS_MEAN / A_SD[abi.P_ABS], np.inf, loc=A_ABS_MEAN, scale=A_SD[abi.P_ABS])
    truth = synth.default_params(synth.make_pack("parsec", 5, n_feh=3, n_age=4, n_eep=25))
    return {abi.P_LOGAGE: (0.5 * (A_AGE[0] + A_AGE[1]), (A_AGE[1] - A_AGE[0]) ** 2 / 12.0),
            abi.P_FEH: (truth[abi.P_FEH], A_SD[abi.P_FEH] ** 2), abi.P_MOD: (truth[abi.P_MOD], A_SD[abi.P_MOD] ** 2),
            abi.P_ABS: (float(tn.mean()), float(tn.var()))}


def target_a_is_constant(marginalised=False, n_rows=200):
    """Before anything else: the log-posterior minus the cluster prior is the same double all over the support (the member
    branch, e^-690 below the field branch, rounds away): every star's value equal bit for bit, the total their sum."""
    pack_d, cl, priors, mean, opt = target_a_problem(marginalised)
    rng = np.random.default_rng(SEED_START)
    rows = np.tile(mean, (n_rows, 1))
    rows[:, abi.P_LOGAGE] = rng.uniform(*A_AGE, n_rows)
    rows[:, abi.P_FEH] += rng.uniform(-5, 5, n_rows) * A_SD[abi.P_FEH]
    rows[:, abi.P_MOD] += rng.uniform(-5, 5, n_rows) * A_SD[abi.P_MOD]
    rows[:, abi.P_ABS] = rng.uniform(0, A_ABS_MEAN + 5 * A_SD[abi.P_ABS], n_rows)
    rows[0, abi.P_LOGAGE], rows[1, abi.P_LOGAGE], rows[2, abi.P_ABS] = A_AGE[0], A_AGE[1], 0.0      # on the walls
    first = None
    for r in rows:
        total, v = numpy_ref.marg_logpost(pack_d, cl, priors, r, 1, 1) if marginalised else numpy_ref.logpost(pack_d, cl, priors, r)
        first = v if first is None else first
        assert np.array_equal(v, first) and np.all(np.isfinite(v))
        assert total == numpy_ref.log_prior_cluster(priors, r, 1) + first.sum()
    return float(first.sum())


def target_a_start(n_walkers):
    pack_d, cl, priors, mean, opt = target_a_problem()
    rng = np.random.default_rng(SEED_START)
    start = np.tile(mean, (n_walkers, 1))
    start[:, abi.P_LOGAGE] = rng.uniform(A_AGE[0] + 0.02, A_AGE[1] - 0.02, n_walkers)
    start[:, abi.P_FEH] += rng.normal(0, 0.02, n_walkers)
    start[:, abi.P_MOD] += rng.normal(0, 0.02, n_walkers)
    start[:, abi.P_ABS] = rng.uniform(0.01, 0.06, n_walkers)
    return start


A_STEPS = (0.03, 0.05, 0.05, 0.03)        # starting proposal sds of DEFAULT_FREE; the burn-in adapts them
A_BURN = 3000


def check_target_a(label, chain, reference=None):
    """chain[step, walker, 4] against target A's analytic moments (or a mutated `reference`), and the six correlations
    against 0.  Returns {name: z} without asserting the thresholds."""
    ref = reference or target_a_moments()
    names = {abi.P_LOGAGE: "log-age", abi.P_FEH: "[Fe/H]", abi.P_MOD: "modulus", abi.P_ABS: "absorption"}
    fig = {}
    for j, k in enumerate(mcmc.DEFAULT_FREE):
        fig[f"{names[k]} mean"], fig[f"{names[k]} var"] = moments(f"{label}, {names[k]}", chain[:, :, j], *ref[k])
    for i in range(4):
        for j in range(i + 1, 4):
            a, b = names[mcmc.DEFAULT_FREE[i]], names[mcmc.DEFAULT_FREE[j]]
            fig[f"corr {a} / {b}"] = correlation_z(f"{label}, {a} / {b}", chain[:, :, i], chain[:, :, j])
    return fig


# ---- problems: the chain, target B (the likelihood in play, one free parameter, flat prior) ---------------------------------
@functools.lru_cache(maxsize=None)
def target_b_problem():
    pack_d, cl, _, _, _, _ = build_problem("parsec", 5, n_stars=120, seed=SEED_CATALOGUE + 1, n_feh=3, n_age=4, n_eep=25)
    # single stars well below the turn-off only: a star near the isochrone's tip or a companion splits the posterior of the
    # age in modes 6 to 18 e-folds apart that a random walk hardly connects -- a property of that target, not of the sampler
    tip = synth.derive_isochrone(pack_d, cl["truth"][abi.P_LOGAGE], cl["truth"][abi.P_FEH], cl["truth"][abi.P_Y])[1][-1]
    cl = subset(cl, np.flatnonzero((np.asarray(cl["mass1"]) < 0.6 * tip) & (np.asarray(cl["mass_ratio"]) == 0) & ~np.asarray(cl["is_field"]))[:40])
    assert len(cl["mass1"]) == 40
    cl["clust_prior"] = np.full(40, 0.9)
    truth = np.array(cl["truth"], dtype=np.float64)
    priors = abi.make_priors(truth, np.zeros(abi.B9_NPARAM), pack_d["log_age"][0], pack_d["log_age"][-1])
    return pack_d, cl, priors, truth


@functools.lru_cache(maxsize=None)
def target_b_reference(k):
    """(mean, variance) of the posterior of parameter k alone, the others at the truth: numpy_ref.logpost on a 2001-point grid
    over mean +- 8 sd, trapezoid rule.  The span is found by two coarse passes of the same kind."""
    pack_d, cl, priors, truth = target_b_problem()

    def on_grid(centre, half, n):
        x = np.linspace(centre - half, centre + half, n)
        lp = np.empty(n)
        for i, v in enumerate(x):
            row = truth.copy(); row[k] = v
            lp[i] = numpy_ref.logpost(pack_d, cl, priors, row)[0]
        top = np.flatnonzero(lp > lp.max() - 1)              # no barrier deeper than 5 e-folds inside the bulk
        assert np.all(lp[top[0]:top[-1] + 1] > lp.max() - 5), "the posterior has modes a random walk does not connect"
        w = np.exp(lp - lp.max())
        norm = _trapz(w, x)
        m = _trapz(w * x, x) / norm
        return m, _trapz(w * (x - m) ** 2, x) / norm

    m, v = on_grid(truth[k], 0.05, 401)
    m, v = on_grid(m, 8 * np.sqrt(v), 401)
    return on_grid(m, 8 * np.sqrt(v), 2001)


def target_b_start(k, n_walkers):
    pack_d, cl, priors, truth = target_b_problem()
    m, v = target_b_reference(k)
    start = np.tile(truth, (n_walkers, 1))
    start[:, k] = m + np.random.default_rng(SEED_START).normal(0, np.sqrt(v), n_walkers)
    return start


B_BURN = 2000
