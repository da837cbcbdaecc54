"""b9_sample_wd_mass (the sampleWDMass counterpart) on the GPU: the draw against the CPU oracle (for n_nodes = 8 K the
drawn node is the one b9o_sample_mass picks at marg_iso_increm = K), against b9_sample_mass, the derived values against the
numpy restatement tests/wd_check.py, bit-for-bit invariances, every kernel instance, edges, and the draw's statistics.
Each test makes its own short-lived engine."""

import numpy as np
import pytest
from scipy import stats

import oracle
import wd_check
from base_amd import abi, synth
from conftest import build_problem
from cli_util import cli as _cli, read_phot as _read_phot

pytestmark = pytest.mark.gpu

PER_STAR = ("obs", "sigma", "mass1", "mass_ratio", "clust_prior", "stage", "wd_type", "is_field", "pop")


def subset(cl, sel):
    """The cluster dict reduced to the stars `sel` (mask or index array)."""
    out = dict(cl)
    for k in PER_STAR:
        out[k] = np.ascontiguousarray(np.asarray(cl[k])[sel])
    return out


def wd_problem(name, n_filt, n_stars, n_y=1, n_pops=1, wd_frac=0.25, seed=12, keep=None, **kw):
    """A catalogue of WD-stage stars only (the stage-3 stars of a synthetic cluster; `keep`: the first so many)."""
    pack_d, cl, pack, _, priors, _ = build_problem(name, n_filt, n_stars=n_stars, wd_frac=wd_frac, n_y=n_y, n_pops=n_pops, seed=seed, **kw)
    idx = np.flatnonzero(np.asarray(cl["stage"]) == abi.STAGE_WD)
    cl = subset(cl, idx if keep is None else idx[:keep])
    return pack_d, cl, pack, abi.make_stars(cl), priors


def rows_for(cl, n_rows, seed, n_pops):
    rows = synth.walker_params(cl["truth"], n_rows, seed=seed, scale=0.3)
    if n_pops == 2:
        rows[:, abi.P_LAMBDA] = np.clip(rows[:, abi.P_LAMBDA], 0.05, 0.95)
    return rows


def opts(n_pops=1, K=1):
    return abi.make_options(mode=abi.MODE_GIVEN_MASS, n_pops=n_pops, marg_iso_increm=K, marg_n_q=1)


def against_oracle(pack_d, cl, pack, stars, priors, n_pops, n_nodes, n_rows, max_left_out=0.001):
    from base_amd import engine
    assert n_nodes % 8 == 0
    rows = rows_for(cl, n_rows, 3, n_pops)
    rows[-1, abi.P_LOGAGE] = pack_d["log_age"][-1] + 1.0                  # a row outside the grid
    eng = engine.Engine(pack, stars, priors, opts(n_pops))
    try:
        g = eng.sample_wd_mass(rows, n_nodes, seed=99, row0=1000)
    finally:
        eng.close()
    om, oq, omem, opop, margin = oracle.Oracle(pack, stars, priors, opts(n_pops, n_nodes // 8)).sample_mass(rows, seed=99, row0=1000)
    assert g["zams"].shape == om.shape and np.array_equal(g["star_index"], np.arange(om.shape[1]))
    for k in ("zams", "member", "wd_mass", "prec_log_age", "log_cool_age", "log_teff", "logg", "pop"):
        assert np.all(g[k][-1] == 0), k
    assert np.all(om[-1] == 0)
    safe = margin > 1e-6
    left_out = 1.0 - safe[:-1].mean()
    print(f"draws left out (oracle margin <= 1e-6): {left_out:.3%}; smallest margin {margin[:-1].min():.3e}; "
          f"distinct masses {len(np.unique(om[:-1]))}")
    assert left_out <= max_left_out
    assert np.array_equal(g["pop"][safe], opop[safe])
    np.testing.assert_allclose(g["zams"][safe], om[safe], rtol=wd_check.ZAMS_RTOL, atol=0)
    np.testing.assert_allclose(g["member"], omem, rtol=1e-9, atol=1e-300)
    return g, om


# ---- 1. the draw equals the oracle's -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_filt,n_y,n_pops,n_nodes", [
    ("parsec", 8, 1, 1, 1024),
    ("dsed", 5, 3, 2, 512),
    ("girardi", 3, 1, 1, 64),
])
def test_draw_equals_oracle(name, n_filt, n_y, n_pops, n_nodes):
    pack_d, cl, pack, stars, priors = wd_problem(name, n_filt, 600, n_y=n_y, n_pops=n_pops)
    assert len(cl["mass1"]) == 150
    g, om = against_oracle(pack_d, cl, pack, stars, priors, n_pops, n_nodes, 7)          # six rows + one outside the grid
    assert len(np.unique(om[:-1])) > 200                                   # the comparison is not vacuous


# ---- 2. equals b9_sample_mass on the WD-stage columns of a mixed catalogue ------------------------------------------------
@pytest.mark.parametrize("K", [1, 3])
def test_equals_sample_mass(K):
    from base_amd import engine
    pack_d, cl, pack, stars, priors, _ = build_problem("dsed", 5, n_stars=300, wd_frac=0.1, n_y=3, n_pops=2, seed=12)
    rows = rows_for(cl, 5, 3, 2)
    eng = engine.Engine(pack, stars, priors, abi.make_options(mode=abi.MODE_GIVEN_MASS, n_pops=2, marg_iso_increm=K, marg_n_q=2))
    try:
        m, q, mem, pop = eng.sample_mass(rows, seed=7, row0=50)
        g = eng.sample_wd_mass(rows, 8 * K, seed=7, row0=50)
    finally:
        eng.close()
    wd = np.flatnonzero(np.asarray(cl["stage"]) == abi.STAGE_WD)
    assert np.array_equal(g["star_index"], wd) and len(wd) == 30
    assert np.array_equal(g["zams"], m[:, wd]) and np.array_equal(g["pop"], pop[:, wd])
    np.testing.assert_allclose(g["member"], mem[:, wd], rtol=1e-12, atol=1e-300)


# ---- 3. the derived values ------------------------------------------------------------------------------------------------
def check_derived(pack_d, cl, rows, g, max_left_out=0.001):
    n_rows, n_wd = g["zams"].shape
    left_out = 0
    for r in range(n_rows):
        for k in np.unique(g["pop"][r]):
            sel = (g["pop"][r] == k) & (g["zams"][r] > 0) & (g["zams"][r] <= pack_d["m_wd_up"])     # (above m_wd_up: no WD, no derived values)
            if not sel.any():
                continue
            wdm, prec, cool, lteff, logg = wd_check.wd_chain(pack_d, rows[r], g["zams"][r, sel], pop=int(k))
            np.testing.assert_allclose(g["wd_mass"][r, sel], wdm, rtol=1e-9, atol=0)
            np.testing.assert_allclose(g["prec_log_age"][r, sel], prec, rtol=1e-9, atol=1e-9)
            # log_cool_age subtracts 10^prec from 10^logAge: where that amplifies an error of prec more than 1e5 times the
            # draw is left out of the comparison of what follows from the cooling age
            t, p = 10.0 ** rows[r, abi.P_LOGAGE], 10.0 ** prec
            ok = ~(t > p) | (t / np.maximum(t - p, 1e-300) <= 1e5)
            left_out += int((~ok).sum())
            for name, want in (("log_cool_age", cool), ("log_teff", lteff), ("logg", logg)):
                np.testing.assert_allclose(g[name][r, sel][ok], want[ok], rtol=1e-9, atol=1e-9, err_msg=name)
    print(f"derived values: {left_out} of {n_rows * n_wd} draws left out (amplification > 1e5)")
    assert left_out <= max_left_out * n_rows * n_wd


@pytest.mark.parametrize("name,n_filt,n_y,n_pops,pack_kw", [
    ("parsec", 8, 1, 1, {}),
    ("dsed", 5, 3, 2, {}),
    ("parsec", 4, 1, 1, {"ragged": False}),
])
def test_derived_values(name, n_filt, n_y, n_pops, pack_kw):
    from base_amd import engine
    pack_d, cl, pack, stars, priors = wd_problem(name, n_filt, 400, n_y=n_y, n_pops=n_pops, **pack_kw)
    rows = rows_for(cl, 5, 3, n_pops)
    eng = engine.Engine(pack, stars, priors, opts(n_pops))
    try:
        g = eng.sample_wd_mass(rows, 512, seed=5)
        check_derived(pack_d, cl, rows, g)
        # the derived values are the ones the likelihood used: the forward model at the drawn mass equals the atmosphere
        # table at the reported (log Teff, log g)
        for r in range(len(rows)):
            died = g["log_teff"][r] != 0
            for k in np.unique(g["pop"][r]):
                sel = (g["pop"][r] == k) & died
                if not sel.any():
                    continue
                wt = np.asarray(cl["wd_type"])[sel]
                mags, stage = eng.predict_mags(rows[r], g["zams"][r, sel], np.zeros(int(sel.sum())), wd_type=wt, pop=np.full(int(sel.sum()), k, np.int32))
                assert np.all(stage == abi.STAGE_WD)
                want = wd_check.apparent(pack_d, rows[r], wd_check.atmosphere_mags(pack_d, g["log_teff"][r, sel], g["logg"][r, sel], wt))
                np.testing.assert_allclose(mags, want, rtol=1e-9, atol=1e-9)
    finally:
        eng.close()


@pytest.mark.parametrize("ifmr_id", [abi.IFMR_WEIDEMANN, abi.IFMR_WILLIAMS, abi.IFMR_SALARIS_LIN, abi.IFMR_SALARIS_PW, abi.IFMR_LINEAR, abi.IFMR_QUADRATIC])
def test_wd_mass_is_the_ifmr_of_zams(ifmr_id):
    from base_amd import engine
    pack_d, cl, _, _, priors, _ = build_problem("parsec", 4, n_stars=200, wd_frac=0.25, seed=12)
    pack_d = dict(pack_d, ifmr_id=ifmr_id)
    cl = subset(cl, np.asarray(cl["stage"]) == abi.STAGE_WD)
    rows = rows_for(cl, 3, 3, 1)
    rows[:, abi.P_IFMR_INTERCEPT], rows[:, abi.P_IFMR_SLOPE], rows[:, abi.P_IFMR_QUAD] = 0.7, 0.1, 0.01
    eng = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cl), priors, opts())
    try:
        g = eng.sample_wd_mass(rows, 256, seed=2)
    finally:
        eng.close()
    assert np.all(g["zams"] > 0)
    for r in range(3):
        np.testing.assert_allclose(g["wd_mass"][r], wd_check.ifmr(pack_d, rows[r], g["zams"][r]), rtol=1e-12, atol=0)


# ---- 4. invariances, bit for bit ------------------------------------------------------------------------------------------
KEYS = ("zams", "wd_mass", "prec_log_age", "log_cool_age", "log_teff", "logg", "member", "pop")


def same(a, b, rows=slice(None)):
    for k in KEYS:
        assert np.array_equal(a[k][rows], b[k]), k


def test_invariances_rows_calls_seed_and_null_outputs():
    from base_amd import engine
    pack_d, cl, pack, stars, priors = wd_problem("parsec", 8, 400)
    rows = rows_for(cl, 40, 8, 1)
    eng = engine.Engine(pack, stars, priors, opts())
    try:
        a = eng.sample_wd_mass(rows, 512, seed=5, row0=0)
        same(a, eng.sample_wd_mass(rows[:7], 512, seed=5, row0=0), slice(0, 7))
        same(a, eng.sample_wd_mass(rows[7:], 512, seed=5, row0=7), slice(7, None))
        same(a, eng.sample_wd_mass(rows, 512, seed=5, row0=0))                       # a repeated call
        lean = eng.sample_wd_mass(rows, 512, seed=5, row0=0, derived=("log_teff",))  # NULL derived outputs
        assert set(lean) == {"zams", "member", "pop", "log_teff", "star_index"}
        for k in ("zams", "member", "pop", "log_teff"):
            assert np.array_equal(lean[k], a[k]), k
        c = eng.sample_wd_mass(rows[:3], 512, seed=6, row0=0)
        assert not np.array_equal(c["zams"], a["zams"][:3])                          # another seed, other draws
        # a grid too fine for 40 rows' tables at once is worked in smaller chunks of rows: same bits as row by row
        fine = eng.sample_wd_mass(rows[:12], 40000, seed=5, row0=3)
        same(fine, eng.sample_wd_mass(rows[5:6], 40000, seed=5, row0=8), slice(5, 6))
    finally:
        eng.close()


def test_outputs_follow_the_stars_when_the_caller_permutes_the_catalogue():
    """The random numbers are keyed by the star's index in the caller's catalogue, so a permuted catalogue draws other
    nodes by definition.  What this test checks is what does not depend on the draw: which stars the columns are
    (star_index) and the membership, bit for bit.  That zams, pop and the derived values land in the right columns of a
    mixed catalogue is test_equals_sample_mass's and test_derived_values' business."""
    from base_amd import engine
    pack_d, cl, pack, stars, priors, _ = build_problem("parsec", 8, n_stars=300, wd_frac=0.2, seed=12)
    rows = rows_for(cl, 4, 8, 1)
    eng = engine.Engine(pack, stars, priors, opts())
    try:
        a = eng.sample_wd_mass(rows, 128, seed=5)
    finally:
        eng.close()
    perm = np.random.default_rng(1).permutation(300)
    eng = engine.Engine(pack, abi.make_stars(subset(cl, perm)), priors, opts())
    try:
        b = eng.sample_wd_mass(rows, 128, seed=5)
    finally:
        eng.close()
    # star perm[j] of the first catalogue is star j of the second; the random numbers follow the star's index, so the
    # draws differ -- what must agree is what does not depend on them: the membership, and which star a column is
    assert np.array_equal(np.sort(perm[b["star_index"]]), a["star_index"])
    col = {s: j for j, s in enumerate(a["star_index"])}
    take = [col[perm[s]] for s in b["star_index"]]
    assert np.array_equal(b["member"], a["member"][:, take])


@pytest.mark.parametrize("n_wd", [1, 63, 64, 65])
def test_star_counts_around_a_wave(n_wd):
    pack_d, cl, pack, stars, priors = wd_problem("parsec", 8, 400, keep=n_wd)
    assert len(cl["mass1"]) == n_wd
    against_oracle(pack_d, cl, pack, stars, priors, 1, 64, 3)


def test_a_star_draws_the_same_whatever_shares_its_wave():
    from base_amd import engine
    pack_d, cl, pack, stars, priors = wd_problem("parsec", 8, 400, keep=65)
    rows = rows_for(cl, 3, 8, 1)
    res = []
    for n in (65, 64, 1):                      # star 0 in a full wave with a second wave behind it, in one wave, alone
        eng = engine.Engine(pack, abi.make_stars(subset(cl, np.arange(n))), priors, opts())
        try:
            res.append(eng.sample_wd_mass(rows, 100, seed=4))
        finally:
            eng.close()
    for k in KEYS:
        assert np.array_equal(res[0][k][:, :64], res[1][k]), k
        assert np.array_equal(res[0][k][:, :1], res[2][k]), k


@pytest.mark.parametrize("n_nodes", [1, 63, 64, 65, 1000])
def test_node_counts_around_a_tile(n_nodes):
    """Any n_nodes: against the numpy statement of the definition (the oracle's grid only has multiples of 8)."""
    from base_amd import engine
    pack_d, cl, pack, stars, priors = wd_problem("parsec", 8, 400, keep=20)
    rows = rows_for(cl, 3, 8, 1)
    eng = engine.Engine(pack, stars, priors, opts())
    try:
        g = eng.sample_wd_mass(rows, n_nodes, seed=4)
        tips = [eng.derive_isochrone(r)[3] for r in rows]
    finally:
        eng.close()
    for r, tip in enumerate(tips):
        dM = (pack_d["m_wd_up"] - tip) / n_nodes
        j = np.rint((g["zams"][r] - tip) / dM)
        assert np.all((j >= 1) & (j <= n_nodes))
        np.testing.assert_allclose(g["zams"][r], tip + dM * j, rtol=1e-13, atol=0)
        terms = node_terms(pack_d, cl, rows[r], tip, n_nodes)                                  # [star][node]
        L = np.logaddexp.reduce(terms, axis=1)
        pm = np.asarray(cl["clust_prior"])
        log_fs = -np.sum(np.log(cl["filter_prior_max"] - cl["filter_prior_min"]))
        with np.errstate(over="ignore"):
            want = 1.0 / (1.0 + np.exp(np.log1p(-pm) + log_fs - np.log(pm) - L))
        # (1e-7, not the project's 1e-9: this numpy statement rebuilds the mass prior's truncation constant from scipy's normal
        #  CDF and the magnitudes from synth's forward model, independent code at ~1e-10 relative on exponents of order 100;
        #  the 1e-9 check of the membership is the oracle's, in against_oracle, for the node counts the oracle's grid has)
        np.testing.assert_allclose(g["member"][r], want, rtol=1e-7, atol=1e-12)
    check_derived(pack_d, cl, rows, g, max_left_out=1.0 if n_nodes == 1 else 0.001)


def node_terms(pack_d, cl, par, tip, n_nodes):
    """term_j of the definition for every star of a WD-only catalogue (one population), in numpy: [star][node]."""
    dM = (pack_d["m_wd_up"] - tip) / n_nodes
    m = tip + dM * np.arange(1, n_nodes + 1)
    obs, sigma = np.asarray(cl["obs"]), np.asarray(cl["sigma"])
    out = np.empty((len(obs), n_nodes))
    lm = np.log(m)
    norm = stats.norm
    zup, zlow = (np.log10(pack_d["m_wd_up"]) + 1.02) / 0.67729, (-1.0 + 1.02) / 0.67729     # oracle: b9o_log_mass_norm
    log_norm = -np.log(0.67729 * np.sqrt(2 * np.pi) * (norm.cdf(zup) - norm.cdf(zlow)))
    lpm = log_norm - 0.5 * ((lm / np.log(10) + 1.02) / 0.67729) ** 2 - lm - np.log(np.log(10))
    for t in (0, 1):
        who = np.flatnonzero(np.asarray(cl["wd_type"]) == t)
        if not len(who):
            continue
        pred = synth.forward_mags(pack_d, par, m, np.zeros(n_nodes), np.full(n_nodes, t))       # [node][f]
        for i in who:
            use = sigma[i] > 0
            z = (pred[:, use] - obs[i, use]) / sigma[i, use]
            out[i] = lpm - 0.5 * np.sum(z * z, axis=1) - np.sum(np.log(sigma[i, use] * np.sqrt(2 * np.pi))) + np.log(dM)
    return out


# ---- 5. every instance ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pops", [1, 2])
@pytest.mark.parametrize("n_filt", [1, 4, 5, 9, 16])
def test_every_instance(n_filt, n_pops):
    pack_d, cl, pack, stars, priors = wd_problem("dsed", n_filt, 400, n_y=3 if n_pops == 2 else 1, n_pops=n_pops, keep=40)
    assert len(cl["mass1"]) == 40
    against_oracle(pack_d, cl, pack, stars, priors, n_pops, 64, 3)


# ---- 6. edges -------------------------------------------------------------------------------------------------------------
def test_no_wd_stage_stars():
    from base_amd import engine
    pack_d, cl, pack, stars, priors, _ = build_problem("parsec", 4, n_stars=50, wd_frac=0.0, seed=4)
    eng = engine.Engine(pack, stars, priors, opts())
    try:
        assert eng.n_wd_stars() == 0
        g = eng.sample_wd_mass(rows_for(cl, 2, 1, 1), 64)
        assert g["zams"].shape == (2, 0) and g["star_index"].size == 0
        with pytest.raises(Exception):
            eng.sample_wd_mass(rows_for(cl, 2, 1, 1), 0)                  # n_nodes < 1: B9_ERR_INVALID
    finally:
        eng.close()


def test_pack_without_wd_tables_follows_the_oracle():
    pack_d, cl, _, _, priors = wd_problem("parsec", 4, 200, keep=30)
    empty = np.zeros(0)
    pack_d = dict(pack_d, wc_carb=empty, wc_mass=empty, wc_log_age=empty, wc_log_teff=empty, wc_log_radius=empty,
                  at_logg=empty, at_log_teff=empty, at_mags=empty, n_at_type=0)
    pack_d.pop("wc_n_age", None); pack_d.pop("wc_offset", None)
    g, _ = against_oracle(pack_d, cl, abi.make_pack(pack_d), abi.make_stars(cl), priors, 1, 64, 3)
    for k in ("wd_mass", "prec_log_age", "log_cool_age", "log_teff", "logg"):
        assert np.all(g[k] == 0)


def test_row_whose_agb_tip_is_not_below_m_wd_up_gives_zeros():
    from base_amd import engine
    pack_d, cl, _, _, priors = wd_problem("parsec", 4, 200, keep=30)
    rows = rows_for(cl, 2, 1, 1)
    pack_d = dict(pack_d, m_wd_up=0.5)                  # below every AGB tip
    eng = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cl), priors, opts())
    try:
        assert eng.derive_isochrone(rows[0])[3] > 0.5
        g = eng.sample_wd_mass(rows, 64)
    finally:
        eng.close()
    for k in KEYS:
        assert np.all(g[k] == 0), k


def test_sampler_blocks_are_untouched():
    from base_amd import engine, mcmc
    pack_d, cl, pack, stars, priors, options = build_problem("parsec", 8, n_stars=400, wd_frac=0.1, seed=4)
    free = np.array(mcmc.DEFAULT_FREE)
    chol = np.diag([mcmc.DEFAULT_STEP[k] for k in free]) * 0.3
    start = synth.walker_params(cl["truth"], 4, seed=2, scale=0.3)
    rows = rows_for(cl, 3, 1, 1)

    def run(interleave):
        eng = engine.Engine(pack, stars, priors, options)
        try:
            lp0 = eng.logpost(start)
            h = eng.mcmc_submit(start, lp0, np.arange(4), free, chol, 11, 0, 6, asynchronous=True)
            if interleave:
                with pytest.raises(Exception) as e:                        # B9_ERR_STATE: a block is outstanding
                    eng.sample_wd_mass(rows, 64)
                assert "outstanding" in str(e.value)
            first = [np.array(x) for x in eng.mcmc_collect(h)[:4]]
            if interleave:
                g = eng.sample_wd_mass(rows, 64)
                assert np.all(g["zams"] > 0)
            h = eng.mcmc_submit(start, lp0, np.arange(4), free, chol, 11, 6, 6, cont=True, asynchronous=True)
            second = [np.array(x) for x in eng.mcmc_collect(h)[:4]]
        finally:
            eng.close()
        return first + second

    for a, b in zip(run(False), run(True)):
        assert np.array_equal(a, b)


# ---- 7. statistics --------------------------------------------------------------------------------------------------------
STAT_SEED = 20240607          # checked on the CPU: the oracle's b9o_sample_mass (K = 32) passes this test's bound with this seed


def stat_problem():
    pack_d, cl, pack, stars, priors = wd_problem("parsec", 8, 400, keep=1)
    rows = np.repeat(rows_for(cl, 1, 3, 1), 4000, axis=0)
    return pack_d, cl, pack, stars, priors, rows


def stat_check(pack_d, cl, rows, zams, tip, n_nodes=256):
    dM = (pack_d["m_wd_up"] - tip) / n_nodes
    j = np.rint((zams - tip) / dM).astype(int)
    assert np.all((j >= 1) & (j <= n_nodes))
    terms = node_terms(pack_d, cl, rows[0], tip, n_nodes)[0]
    prob = np.exp(terms - np.logaddexp.reduce(terms))
    expect = prob * len(zams)
    count = np.bincount(j - 1, minlength=n_nodes).astype(float)
    big = expect >= 5
    obs_c, exp_c = list(count[big]), list(expect[big])
    if (~big).any():                                    # the nodes with small expected counts, pooled
        obs_c.append(count[~big].sum()); exp_c.append(expect[~big].sum())
    obs_c, exp_c = np.array(obs_c), np.array(exp_c)
    keep = exp_c > 0
    chi2 = np.sum((obs_c[keep] - exp_c[keep]) ** 2 / exp_c[keep])
    dof = int(keep.sum()) - 1
    p = stats.chi2.sf(chi2, dof) if dof > 0 else 1.0
    print(f"goodness of fit: chi2 {chi2:.2f}, {dof} degrees of freedom, p {p:.4f}, {int(big.sum())} nodes with expected count >= 5")
    assert dof >= 3, "the posterior sits on too few nodes for the test to say anything"
    assert p > 1e-4
    return p


def test_draws_follow_the_categorical_posterior():
    from base_amd import engine
    pack_d, cl, pack, stars, priors, rows = stat_problem()
    eng = engine.Engine(pack, stars, priors, opts())
    try:
        g = eng.sample_wd_mass(rows, 256, seed=STAT_SEED)
        tip = eng.derive_isochrone(rows[0])[3]
    finally:
        eng.close()
    stat_check(pack_d, cl, rows, g["zams"][:, 0], tip)


# ---- 8. the CLI loop ------------------------------------------------------------------------------------------------------
WD_FILES = ("zamsMass", "mass", "precLogAge", "coolingAge", "logTeff", "logg", "membership")
WD_KEYS = ("zams", "wd_mass", "prec_log_age", "log_cool_age", "log_teff", "logg", "member")


def test_cli_loop_files_equal_the_engine_and_recover_the_simulated_masses(tmp_path):
    """simCluster (seeded, WD primaries) -> scatterCluster -> singlePopMcmc (short) -> sampleWDMass.  Every step runs under
    its own time limit and a failed step ends the test."""
    from base_amd import build, engine, host_build, hostlib
    build.build_hip()
    host_build.build_host()
    n_nodes = 256
    pack_d = synth.make_pack("parsec", 8, n_feh=4, n_age=8, n_eep=90)
    truth = synth.default_params(pack_d)
    truth[abi.P_IFMR_INTERCEPT], truth[abi.P_IFMR_SLOPE], truth[abi.P_IFMR_QUAD] = 0.77, 0.08, 0.0   # the session's defaults
    root = synth.write_models_dir(pack_d, str(tmp_path / "models"))
    base = str(tmp_path / "run")
    y_true = synth.write_yaml(str(tmp_path / "truth.yaml"), base + ".sim.scatter", root, base, truth, seed=17)
    r = _cli("simCluster", "--config", y_true, "--nStars", "1500", "--percentBinary", "20", "--percentDB", "20", "--minMass", "0.6")
    assert r.returncode == 0, r.stderr
    r = _cli("scatterCluster", "--config", y_true, "--sigmaFloor", "0.01", "--sigmaAtLimit", "0.05", "--faintLimit", "45")
    assert r.returncode == 0, r.stderr
    start = truth.copy()
    start[abi.P_LOGAGE] += 0.004; start[abi.P_MOD] += 0.01; start[abi.P_FEH] -= 0.01
    fit = str(tmp_path / "fit")
    y = synth.write_yaml(str(tmp_path / "fit.yaml"), base + ".sim.scatter", root, fit, start, burn=3000, run=300, walkers=4)
    r = _cli("singlePopMcmc", "--config", y, "--priorFe_H", repr(float(truth[abi.P_FEH])), "--priorDistMod", repr(float(truth[abi.P_MOD])),
             "--priorAv", repr(float(truth[abi.P_ABS])))
    assert r.returncode == 0, r.stderr
    r = _cli("sampleWDMass", "--config", y, "--nMassNodes", str(n_nodes), "--seed", "31")
    assert r.returncode == 0, r.stderr
    assert "star draws/s" in r.stderr and "%d mass nodes" % n_nodes in r.stderr

    # seven files: a header of the WD-stage stars' ids in .phot order, one line per stage-3 row
    cl = _read_phot(base + ".sim.scatter")
    ids = [ln.split()[0] for ln in open(base + ".sim.scatter").read().splitlines()[1:]]
    wd = np.flatnonzero(cl["stage"] == abi.STAGE_WD)
    assert len(wd) >= 100
    rows = hostlib.read_res_rows(fit + ".res", start, 3)
    assert len(rows) == 300 * 4
    eng = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cl), synth.default_priors(pack_d, truth), opts())
    try:
        g = eng.sample_wd_mass(rows, n_nodes, seed=31, row0=0)
        tip = eng.derive_isochrone(truth)[3]
    finally:
        eng.close()
    assert np.array_equal(g["star_index"], wd)
    files = {}
    for kind, key in zip(WD_FILES, WD_KEYS):
        path = fit + ".wd." + kind
        assert open(path).readline().split() == [ids[i] for i in wd], kind
        files[key] = np.loadtxt(path, skiprows=1, ndmin=2)
        assert files[key].shape == (len(rows), len(wd)), kind
        np.testing.assert_allclose(files[key], g[key], rtol=0, atol=6e-7, err_msg=kind)        # %.6f

    # recovery against the truth in .sim.out: the true ZAMS mass inside the 0.5 % .. 99.5 % quantiles of the star's draws,
    # widened by one node spacing
    sim = open(base + ".sim.out").read().splitlines()
    col = {n: i for i, n in enumerate(sim[0].split())}
    true_mass = {ln.split()[0]: float(ln.split()[col["mass1"]]) for ln in sim[1:]}
    spacing = (pack_d["m_wd_up"] - tip) / n_nodes
    lo, hi = np.quantile(files["zams"], [0.005, 0.995], axis=0)
    m_true = np.array([true_mass[ids[i]] for i in wd])
    inside = (m_true >= lo - spacing) & (m_true <= hi + spacing)
    print(f"recovery: {inside.mean():.1%} of {len(wd)} simulated WDs have their true ZAMS mass inside the 99 % interval of their draws "
          f"(node spacing {spacing:.4f} Msun; median interval width {np.median(hi - lo):.4f} Msun)")
    assert inside.mean() >= 0.9

    # a catalogue without WD-stage stars is an error with a clear message
    r = _cli("simCluster", "--config", y_true, "--nStars", "60", "--minMass", "0.6", "--maxMass", "1.0")
    assert r.returncode == 0, r.stderr
    r = _cli("scatterCluster", "--config", y_true, "--sigmaFloor", "0.01", "--sigmaAtLimit", "0.05", "--faintLimit", "45")
    assert r.returncode == 0, r.stderr
    r = _cli("sampleWDMass", "--config", y, "--nMassNodes", str(n_nodes))
    assert r.returncode != 0 and "no WD-stage star" in r.stderr
    r = _cli("sampleWDMass", "--config", y, "--nMassNodes", "0")
    assert r.returncode != 0
