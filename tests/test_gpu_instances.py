"""Every template instance the kernels dispatch to at run time (B9_SWITCH_NFP: padded filter width NFP 4 / 8 / 16 x one or
two populations; the marginalised star kernel's sparse-split, split, tiled and scalar launch forms; the fused marginalised
step and its two-launch fallback; node tables longer than the level-1 mask) checked against the oracle, the numpy
restatement or the host twin of the sampler.

Which instance a shape takes: NFP = 4 for 1-4 filters, 8 for 5-8, 16 for 9-16.  A marginalised catalogue of n_mc 64-star
chunks (WD-stage stars apart) is SPLIT when n_mc x n_pops < 512 (b9k_marg_split), and a split launch is SPARSE when its
pieces x walkers <= 5 x CUs (marg_sparse); an unsplit catalogue runs the TILED star kernel at NFP = 16 or with two
populations, the SCALAR one otherwise (launch_star_marg_t, launch_marg_step).  sampleMass draws never split."""
import numpy as np
import pytest

import oracle
from base_amd import abi, engine, hostlib, mcmc, synth
from chain_check import oracle_delta
from placement_check import launch_form as _launch_form, n_cu as _n_cu, plan_pieces as _plan_pieces  # noqa: F401  (shared with tests/test_gpu_placement.py)
from sim_check import branch_systems, forward_by_pop, isochrone_tips
import numpy_ref

pytestmark = pytest.mark.gpu

MSTEP_SEC_ROWS = 24                        # b9_marg_step.hip.h: B9_MSTEP_SEC_ROWS


def _nfp(n_filt):
    return 4 if n_filt <= 4 else (8 if n_filt <= 8 else 16)


def _mass_cap(eng):
    return (eng.max_eep() + 1) & ~1


def _fused_limit(nfp):
    """The longest mass column (doubles) k_marg_step takes: b9k_marg_step_lds <= B9_MSTEP_LDS_MAX (marg_fused_ok)."""
    lds_max = (30 if nfp > 8 else 15) * 1024 // 8
    return lds_max - 8 - 65 * nfp - 4 * MSTEP_SEC_ROWS * nfp


def _free(n_pops):
    return np.array(list(mcmc.DEFAULT_FREE) + ([abi.P_Y, abi.P_Y2, abi.P_LAMBDA] if n_pops == 2 else []))


def _chol(n_pops, scale=1.0):
    return np.diag([3e-3, 2e-2, 8e-3, 6e-3] + ([2e-3, 2e-3, 2e-2] if n_pops == 2 else [])) * scale


def _rel(got, want):
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin)
    return float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))))


def _drop_filters(cl, seed):
    """Unused filters (sigma <= 0) on some stars; with more than 8 filters in the upper half of the 16-wide row."""
    rng = np.random.default_rng(seed)
    sg = np.array(cl["sigma"], dtype=np.float64)
    n, nf = sg.shape
    for i in range(0, n, 5):
        if nf > 8:
            sg[i, 8 + rng.integers(nf - 8)] = -1.0
            if i % 3 == 0:
                sg[i, nf - 1] = -1.0
        else:
            sg[i, rng.integers(nf)] = -1.0
    cl["sigma"] = sg
    return cl


def _problem(n_filt, n_pops, n_stars, seed, wd_frac=0.0, name=None, **pack_kw):
    kw = dict(n_feh=3, n_age=6, n_eep=48)
    kw.update(pack_kw)
    name = name or ("dsed" if n_pops == 2 else "parsec")
    pack_d = synth.make_pack(name, n_filt, n_y=3 if n_pops == 2 else 1, **kw)
    truth = synth.default_params(pack_d)
    cl = _drop_filters(synth.make_cluster(pack_d, n_stars, seed=seed, truth=truth, wd_frac=wd_frac, n_pops=n_pops), seed)
    return pack_d, cl, abi.make_pack(pack_d), abi.make_stars(cl), synth.default_priors(pack_d, truth, n_pops)


def _start(cl, W, n_pops, seed=3, scale=0.1):
    return synth.walker_params(cl["truth"], W, seed=seed, scale=scale, n_pops=n_pops)


def _twin_check(eng, orc, start, n_pops, n_steps, seed, scale=1.0, oracle_walkers=None, exact=False):
    """The device block (whatever step the engine's mode and shape pick) against the host twin over the engine's own
    log-posterior, then every distinct recorded state (of the first `oracle_walkers` walkers) against the oracle.  Positions
    to 1e-12 (the twin's normals come from numpy's log / sin / cos), or bit for bit with `exact`."""
    W = start.shape[0]
    free, chol = _free(n_pops), _chol(n_pops, scale)
    lp0 = eng.logpost(start)
    host = mcmc.HostBlockRunner(eng.logpost).run(start, lp0, np.arange(W), free, chol, seed, 0, n_steps)
    dev = mcmc.DeviceBlockRunner(eng).run(start, lp0, np.arange(W), free, chol, seed, 0, n_steps)
    assert dev[4] == host[4] and dev[4] > 0, (dev[4], host[4])
    if exact:
        np.testing.assert_array_equal(dev[2], host[2])
    np.testing.assert_allclose(dev[2], host[2], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(dev[3], host[3], rtol=1e-10)
    worst = 0.0
    for w in range(min(W, oracle_walkers or W)):
        err, _ = oracle_delta(orc, start[w], free, dev[2][:, w], dev[3][:, w])
        worst = max(worst, err)
    assert worst <= 1e-9, worst
    return dev


def _sample_mass_check(eng, orc, cl, rows, seed=99):
    """sampleMass against the oracle's restatement: exact mass ratio and population where the two best keys are apart,
    mass to 1e-12, membership to 1e-9; WD-stage stars draw without a companion."""
    gm, gq, gmem, gpop = eng.sample_mass(rows, seed=seed, row0=500)
    om, oq, omem, opop, margin = orc.sample_mass(rows, seed=seed, row0=500)
    safe = margin > 1e-6
    assert safe.mean() > 0.999
    assert np.array_equal(gpop[safe], opop[safe])
    np.testing.assert_allclose(gq[safe], oq[safe], rtol=0, atol=0)
    np.testing.assert_allclose(gm[safe], om[safe], rtol=1e-12, atol=0)
    np.testing.assert_allclose(gmem, omem, rtol=1e-9, atol=1e-300)
    wd = np.asarray(cl["stage"]) == abi.STAGE_WD
    if wd.any():
        assert np.all(gq[:, wd] == 0)
    return gm, gq, gmem, gpop


def _mass_rows(cl, n, n_pops, seed=3):
    rows = synth.walker_params(cl["truth"], n, seed=seed, scale=0.3, n_pops=n_pops)
    if n_pops == 2:
        rows[:, abi.P_LAMBDA] = np.clip(rows[:, abi.P_LAMBDA], 0.05, 0.95)
    return rows


# ---------------------------------------------------------------------------------------------------------------------------
# A. the fused marginalised step at the full size of the BASELINE configurations
# ---------------------------------------------------------------------------------------------------------------------------
def _pick_states(samples, cap):
    """(step, walker) of at most `cap` distinct recorded states: the last state, the first state after a move, and the rest
    spread evenly over the chain."""
    n, W, _ = samples.shape
    seen, order = set(), []
    for t in range(n):
        for w in range(W):
            key = samples[t, w].tobytes()
            if key not in seen:
                seen.add(key)
                order.append((t, w))
    moved = [(t, w) for t, w in order if t > 0]
    pick = [(n - 1, 0)] + moved[:1]
    rest = [o for o in order if o not in pick]
    if rest:
        for i in np.unique(np.linspace(0, len(rest) - 1, max(0, cap - len(pick))).round().astype(int)):
            pick.append(rest[i])
    return pick[:cap], len(moved)


@pytest.mark.parametrize("name,walkers", [("C1", 1), ("C2", 2), ("C3", 1), ("C4", 4)])
def test_fused_marginalised_sampler_matches_oracle_full_size(name, walkers):
    """k_marg_step driven by the C++ sampler (b9h::WalkerSampler, pipelined device-resident blocks) in marginalised mode at
    K = Q = 4 on the FULL BASELINE catalogues: C1 (10k stars: split into pieces + k_marg_step_merge), C2 (50k: unsplit),
    C3 (20k with 5% WD-stage stars: the WD-table builder role), C4 (30k, two populations with Y, Y2 and lambda free: the
    eight-corner tables).  Up to six distinct recorded states per configuration (the last one and one after a move among
    them) and the ensemble state the sampler reports equal the oracle's brute-force integral to 1e-9 relative."""
    cfg = synth.make_baseline_config(name)
    n_pops, free = cfg["n_pops"], cfg["free"]
    opt = abi.make_options(abi.MODE_MARGINALISED, n_pops, 4, 4)
    eng = engine.Engine(cfg["pack"], cfg["stars"], cfg["priors"], opt)
    if name == "C3":
        assert (np.asarray(cfg["cluster"]["stage"]) == abi.STAGE_WD).sum() > 500
    if name == "C4":
        assert n_pops == 2 and set(free) >= {abi.P_Y, abi.P_Y2, abi.P_LAMBDA}
    assert _mass_cap(eng) <= _fused_limit(8), "this pack no longer takes the fused step"
    start = synth.walker_params(cfg["truth"], walkers, seed=7, n_pops=n_pops, scale=0.02)
    step = [mcmc.DEFAULT_STEP[k] * 0.3 for k in free]
    s = hostlib.HostSampler(walkers, free, step, hostlib.Exchange.local(), seed=11, block=4, engine=eng)
    s.initialise(start)
    a = s.run(8, adapt=True, record=True)
    b = s.run(8, adapt=False, record=True)
    samples, lps = np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])
    assert samples.shape == (16, walkers, len(free))
    pick, n_moved = _pick_states(samples, 6)
    assert n_moved > 0, "no walker moved: only the starting state would be checked"
    st = s.state()
    rows = np.repeat(start[:1], len(pick) + walkers, axis=0)
    for i, (t, w) in enumerate(pick):
        rows[i] = start[w]
        rows[i, list(free)] = samples[t, w]
    rows[len(pick):] = st["all_params"]
    want = oracle.Oracle(cfg["pack"], cfg["stars"], cfg["priors"], opt, native=True).logpost(rows)
    got = np.concatenate([[lps[t, w] for t, w in pick], st["all_logpost"]])
    assert np.all(np.isfinite(want))
    assert _rel(got, want) <= 1e-9, (name, got, want)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------------
# B. the instance matrix: 1, 4, 5, 9, 16 filters x one and two populations
# ---------------------------------------------------------------------------------------------------------------------------
MATRIX = [(nf, npop) for nf in (1, 4, 5, 9, 16) for npop in (1, 2)]


def _matrix_problem(n_filt, n_pops):
    return _problem(n_filt, n_pops, 96, seed=100 + 10 * n_filt + n_pops, wd_frac=0.08)


@pytest.mark.parametrize("n_filt,n_pops", MATRIX)
def test_given_mass_instances(monkeypatch, n_filt, n_pops):
    """b9_logpost (k_star_like<NFP, NPOPS>) per star against the oracle, then the fused one-step launch (k_mcmc_step, depth 1)
    and the tree launch (k_mcmc_tree, depth 2 and 3) against the host twin."""
    pack_d, cl, pack, stars, priors = _matrix_problem(n_filt, n_pops)
    opt = abi.make_options(abi.MODE_GIVEN_MASS, n_pops)
    orc = oracle.Oracle(pack, stars, priors, opt)
    eng = engine.Engine(pack, stars, priors, opt)
    rows = _start(cl, 3, n_pops, seed=5, scale=0.5)
    lp_g, ps_g = eng.logpost(rows, perstar=True)
    lp_o, ps_o = orc.logpost(rows, perstar=True)
    assert _rel(ps_g, ps_o) <= 1e-9 and _rel(lp_g, lp_o) <= 1e-9
    W = 3
    start = _start(cl, W, n_pops)
    free, chol = _free(n_pops), _chol(n_pops, 0.3)
    lp0 = eng.logpost(start)
    host = mcmc.HostBlockRunner(eng.logpost).run(start, lp0, np.arange(W), free, chol, 5, 0, 12)
    assert host[4] > 0
    eng.close()
    for depth in (1, 2, 3):
        monkeypatch.setenv("B9_TREE_DEPTH", str(depth))
        e = engine.Engine(pack, stars, priors, opt)
        assert e.step_depth(W) == depth
        dev = mcmc.DeviceBlockRunner(e).run(start, lp0, np.arange(W), free, chol, 5, 0, 12)
        assert dev[4] == host[4], depth
        np.testing.assert_allclose(dev[2], host[2], rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(dev[3], host[3], rtol=1e-10)
        e.close()


@pytest.mark.parametrize("n_filt,n_pops", MATRIX)
def test_marginalised_instances(n_filt, n_pops):
    """Marginalised b9_logpost (k_marg_table, k_star_marg, k_marg_wd_table, k_star_marg_wd at this NFP; 96 stars: a split,
    sparse catalogue) per star and in total against the oracle -- and at 9 and 16 filters against tests/numpy_ref.py, which
    shares no code with it -- then the fused sampler step (k_marg_step) against the host twin and the oracle."""
    pack_d, cl, pack, stars, priors = _matrix_problem(n_filt, n_pops)
    K, Q = 2, 3
    opt = abi.make_options(abi.MODE_MARGINALISED, n_pops, K, Q)
    eng = engine.Engine(pack, stars, priors, opt)
    orc = oracle.Oracle(pack, stars, priors, opt)
    wd = np.asarray(cl["stage"]) == abi.STAGE_WD
    assert wd.sum() >= 4
    rows = _start(cl, 3, n_pops, seed=5, scale=0.5)
    lp_g, ps_g = eng.logpost(rows, perstar=True)
    lp_o, ps_o = orc.logpost(rows, perstar=True)
    assert np.isfinite(ps_o).mean() > 0.9
    assert _rel(ps_g, ps_o) <= 1e-9 and _rel(lp_g, lp_o) <= 1e-9
    if n_filt > 8:
        assert len(cl["mass1"]) <= 100
        lp_n, ps_n = numpy_ref.marg_logpost(pack_d, cl, priors, rows[0], K, Q, n_pops)
        assert _rel(ps_g[0], ps_n) <= 1e-9 and _rel(lp_g[:1], np.array([lp_n])) <= 1e-9
    assert _mass_cap(eng) <= _fused_limit(_nfp(n_filt))
    _twin_check(eng, orc, _start(cl, 3, n_pops), n_pops, 10, seed=7, scale=0.3)
    eng.close()


@pytest.mark.parametrize("n_filt,n_pops", MATRIX)
def test_sample_mass_instances(n_filt, n_pops):
    """sampleMass (k_star_marg<NFP, NPOPS, SAMPLE = true>, k_star_marg_wd<NFP, NPOPS, true>) against Oracle.sample_mass."""
    pack_d, cl, pack, stars, priors = _matrix_problem(n_filt, n_pops)
    opt = abi.make_options(abi.MODE_MARGINALISED, n_pops, 2, 3)
    eng = engine.Engine(pack, stars, priors, opt)
    _sample_mass_check(eng, oracle.Oracle(pack, stars, priors, opt), cl, _mass_rows(cl, 4, n_pops))
    eng.close()


@pytest.mark.parametrize("n_filt,n_pops", [(1, 1), (4, 2), (9, 1), (16, 2), (16, 1)])
def test_predict_mags_instances(n_filt, n_pops):
    """b9_predict_mags (k_predict_mags<NFP>) against synth.forward_mags on every branch of tests/test_gpu_sim.py's systems:
    dark systems exactly MAG_NOFLUX, lit ones to 1e-10."""
    pack_d = synth.make_pack("dsed" if n_pops == 2 else "parsec", n_filt, n_y=3 if n_pops == 2 else 1, n_feh=4, n_age=8, n_eep=90)
    row = synth.default_params(pack_d)
    pack = abi.make_pack(pack_d)
    isos = isochrone_tips(pack, row, n_pops)
    m1, q, wt, pop = branch_systems(isos, pack_d["m_wd_up"], n_pops, np.random.default_rng(n_filt))
    eng = engine.Engine(pack)
    mags, stage = eng.predict_mags(row, m1, q, wt, pop if n_pops == 2 else None)
    assert mags.shape == (len(m1), n_filt)
    want = forward_by_pop(pack_d, row, m1, q, wt, pop)
    first = np.array([isos[k][1][0] for k in pop])
    dark = ((m1 < first) | (m1 > pack_d["m_wd_up"])) & ((q == 0) | (q * m1 < first))
    assert dark.sum() >= 3 * n_pops and (~dark).sum() >= 80 * n_pops
    assert np.all(mags[dark] == abi.MAG_NOFLUX)
    np.testing.assert_allclose(mags[~dark], want[~dark], rtol=0, atol=1e-10)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------------
# C. catalogue sizes that pick each launch form of the marginalised kernels
# ---------------------------------------------------------------------------------------------------------------------------
def _catalogue_case(capfd, n_filt, n_pops, n_stars, W, want_form, seed, steps=6):
    pack_d, cl, pack, stars, priors = _problem(n_filt, n_pops, n_stars, seed=seed, n_feh=3, n_age=5, n_eep=40)
    opt = abi.make_options(abi.MODE_MARGINALISED, n_pops, 2, 2)
    eng = engine.Engine(pack, stars, priors, opt)
    orc = oracle.Oracle(pack, stars, priors, opt, native=True)
    start = _start(cl, W, n_pops)
    form, (lp_g, ps_g) = _launch_form(eng, start, W, n_pops, cl, _n_cu(capfd), capfd)
    if want_form is not None:
        assert form == want_form, (form, want_form)
    k = min(W, 3)
    lp_o, ps_o = orc.logpost(start[:k], perstar=True)
    assert _rel(ps_g[:k], ps_o) <= 1e-9 and _rel(lp_g[:k], lp_o) <= 1e-9
    _twin_check(eng, orc, start, n_pops, steps, seed=13, scale=0.3, oracle_walkers=2)
    _sample_mass_check(eng, orc, cl, _mass_rows(cl, 2, n_pops))
    eng.close()
    return form


@pytest.mark.parametrize("n_filt,n_pops,n_stars,W,form", [
    (4, 1, 2000, 1, "sparse"), (16, 1, 2000, 1, "sparse"), (16, 2, 2000, 1, "sparse"),
    (4, 1, 2000, 48, "split"), (16, 1, 2000, 48, "split"), (16, 2, 2000, 48, "split"),
    (4, 1, 32768, 2, "scalar"), (16, 1, 32768, 2, "tiled"), (16, 2, 16384, 2, "tiled"),
])
def test_launch_forms(capfd, n_filt, n_pops, n_stars, W, form):
    """Each launch form of k_star_marg and k_marg_step at NFP 4 and 16: SPARSE split (one chain on 2000 stars: at most 32
    pieces x 32 chunks <= 5 x CUs), SPLIT (48 chains: pieces x walkers >= 32 x 48 > 5 x CUs), unsplit SCALAR (NFP 4, one
    population, 512 chunks) and unsplit TILED (NFP 16: 512 chunks of one population, 256 of two).  Split or not is read back
    from the catalogue plan (its piece count); sparse against split and tiled against scalar follow from the piece count, the
    walkers, the library's CU count and NFP by the rules of marg_sparse and launch_star_marg_t, restated here.  Log-posteriors against the oracle, the fused step's chain against the host twin and the oracle,
    sampleMass (never split: its own unsplit instances) against the oracle."""
    _catalogue_case(capfd, n_filt, n_pops, n_stars, W, form, seed=n_stars + n_filt + n_pops)


@pytest.mark.parametrize("n_filt,n_pops", [(4, 1), (16, 2)])
@pytest.mark.parametrize("n_stars", [1, 63, 64, 65, 257])
def test_star_counts_at_chunk_edges(capfd, n_filt, n_pops, n_stars):
    """Catalogues of one star, one chunk less / exactly / one more, and four chunks plus one (split sparse launches with
    half-empty waves and chunks whose lanes are mostly padding)."""
    form = _catalogue_case(capfd, n_filt, n_pops, n_stars, 2, None, seed=n_stars)
    assert form == "sparse"


@pytest.mark.parametrize("n_filt,n_pops,edge", [(4, 1, 32704), (16, 2, 16320)])
@pytest.mark.parametrize("side", [0, 1])
def test_split_threshold(capfd, n_filt, n_pops, edge, side):
    """One catalogue just below the split threshold (511 chunks of one population, 255 of two: split) and one just above
    (one star more: 512 / 256 chunks, unsplit: scalar at NFP 4, tiled at NFP 16)."""
    form = _catalogue_case(capfd, n_filt, n_pops, edge + side, 2, None, seed=7 + side)
    if side == 0:
        assert form in ("sparse", "split")
    else:
        assert form == ("scalar" if n_filt == 4 else "tiled")


# ---------------------------------------------------------------------------------------------------------------------------
# D. the fused step's LDS limit and node tables longer than the level-1 mask
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_filt", [4, 8, 16])
@pytest.mark.parametrize("side", ["under", "over"])
def test_fused_step_lds_limit(n_filt, side):
    """Packs whose mass column just fits the fused step's LDS budget (k_marg_step) and just does not (the two-launch step,
    marg_fused_ok false): the marginalised chain is the host twin's (positions bit for bit) and the oracle's either way."""
    nfp = _nfp(n_filt)
    limit = _fused_limit(nfp)
    n_eep = limit if side == "under" else limit + 2
    pack_d, cl, pack, stars, priors = _problem(n_filt, 1, 120, seed=n_eep, wd_frac=0.05, n_feh=3, n_age=4, n_eep=n_eep)
    opt = abi.make_options(abi.MODE_MARGINALISED, 1, 1, 2)
    eng = engine.Engine(pack, stars, priors, opt)
    cap = _mass_cap(eng)
    assert (cap <= limit) == (side == "under"), (cap, limit)
    assert abs(cap - limit) <= 2
    _twin_check(eng, oracle.Oracle(pack, stars, priors, opt), _start(cl, 3, 1), 1, 8, seed=3, scale=0.3, exact=True)
    eng.close()


def _n_chunks(eng, row, K):
    n = eng.derive_isochrone(row, 0, cap=_mass_cap(eng))[1].size
    return ((n - 1) * K + 63) // 64


MASK_NODES = 64 * 1024                     # 64 nodes per chunk x 64 x B9_MARG_MASK_WORDS chunks under the level-1 mask


def _stars_past_the_mask(pack_d, cl, K, n_put=6):
    """Move `n_put` single, non-WD stars onto the upper giant branch, past node MASK_NODES of the truth's node table (the
    chunks only the loop after the mask reaches), with photometry that the nodes before it cannot explain: every node
    under the mask lies at least chi^2 = 100 away from each of them, so their likelihood is all in the tail.  Returns the
    stars' indices."""
    t = cl["truth"]
    _, mass, _ = synth.derive_isochrone(pack_d, t[abi.P_LOGAGE], t[abi.P_FEH], t[abi.P_Y])
    e_cut = MASK_NODES // K + 1
    assert e_cut < len(mass) - 1, "the node table does not reach past the mask"
    m = np.linspace(mass[e_cut], mass[-1], n_put + 2)[1:-1]
    idx = np.flatnonzero(np.asarray(cl["stage"]) != abi.STAGE_WD)[1:2 * n_put:2]
    pred = synth.forward_mags(pack_d, t, m, np.zeros(n_put), np.zeros(n_put, np.int32))
    for k, v in (("mass1", m), ("mass_ratio", 0.0), ("clust_prior", 0.95)):
        cl[k][idx] = v
    cl["obs"][idx] = pred
    cl["sigma"][idx] = 0.02
    cl["filter_prior_min"] = np.minimum(cl["filter_prior_min"], pred.min(axis=0) - 0.5)
    cl["filter_prior_max"] = np.maximum(cl["filter_prior_max"], pred.max(axis=0) + 0.5)
    # the nodes under the mask (primary masses mass[e] + s (mass[e+1] - mass[e]) / K, single stars)
    e = np.arange(MASK_NODES) // K
    nodes = mass[e] + (np.arange(MASK_NODES) % K) * ((mass[e + 1] - mass[e]) / K)
    head = synth.forward_mags(pack_d, t, nodes, np.zeros(MASK_NODES), np.zeros(MASK_NODES, np.int32))
    chi2 = (((head[:, None, :] - pred[None, :, :]) / 0.02) ** 2).sum(axis=2).min(axis=0)
    assert np.all(chi2 > 100), chi2
    return idx


@pytest.mark.parametrize("n_filt,n_eep,K,tail", [(8, 2000, 40, True), (4, 2048, 32, False)])
def test_node_tables_past_the_mask(n_filt, n_eep, K, tail):
    """Node tables of more than 64 x B9_MARG_MASK_WORDS = 1024 chunks (2000 EEPs x K = 40: the chunks past the level-1 mask
    are tested by every wave, and six stars on the upper giant branch have their likelihood there) and of exactly 1024 (2048
    EEPs x 32): b9_logpost and sampleMass against the oracle, and the pruned kernel against the same kernel evaluating
    every node."""
    pack_d, cl, pack, stars, priors = _problem(n_filt, 1, 64, seed=K, wd_frac=0.05, ragged=False, n_feh=3, n_age=4, n_eep=n_eep)
    if tail:
        _stars_past_the_mask(pack_d, cl, K)
        stars = abi.make_stars(cl)
    opt = abi.make_options(abi.MODE_MARGINALISED, 1, K, 1)
    eng = engine.Engine(pack, stars, priors, opt)
    rows = _start(cl, 2, 1, seed=4, scale=0.5)
    n_ch = _n_chunks(eng, rows[0], K)
    assert (n_ch > 1024) if tail else (n_ch == 1024), n_ch
    orc = oracle.Oracle(pack, stars, priors, opt, native=True)
    lp_g, ps_g = eng.logpost(rows, perstar=True)
    lp_o, ps_o = orc.logpost(rows, perstar=True)
    assert _rel(ps_g, ps_o) <= 1e-9 and _rel(lp_g, lp_o) <= 1e-9
    draws = _sample_mass_check(eng, orc, cl, _mass_rows(cl, 2, 1))
    eng.set_tuning(marg_no_pruning=1)
    lp_b, ps_b = eng.logpost(rows, perstar=True)
    draws_b = eng.sample_mass(_mass_rows(cl, 2, 1), seed=99, row0=500)
    eng.set_tuning()
    assert _rel(ps_g, ps_b) <= 1e-12
    np.testing.assert_allclose(lp_g, lp_b, rtol=1e-12)
    np.testing.assert_allclose(draws[2], draws_b[2], rtol=1e-12, atol=1e-300)
    eng.close()


@pytest.mark.parametrize("n_filt,n_eep,K", [(8, 600, 112), (16, 1200, 56)])
def test_fused_step_with_tables_past_the_mask(n_filt, n_eep, K):
    """The fused step (k_marg_step; still inside its LDS budget) on node tables of more than 1024 chunks, built by its own
    table role (marg_build_table), with six stars whose likelihood lies in the chunks past the level-1 mask: its chain against
    the host twin and the oracle, and against the same step evaluating every node (positions equal, log-posteriors to
    1e-12)."""
    pack_d, cl, pack, stars, priors = _problem(n_filt, 1, 64, seed=K, ragged=False, n_feh=3, n_age=4, n_eep=n_eep)
    _stars_past_the_mask(pack_d, cl, K)
    stars = abi.make_stars(cl)
    opt = abi.make_options(abi.MODE_MARGINALISED, 1, K, 1)
    eng = engine.Engine(pack, stars, priors, opt)
    assert _mass_cap(eng) <= _fused_limit(_nfp(n_filt))
    start = _start(cl, 2, 1)
    assert _n_chunks(eng, start[0], K) > 1024
    dev = _twin_check(eng, oracle.Oracle(pack, stars, priors, opt, native=True), start, 1, 6, seed=9, scale=0.3)
    eng.set_tuning(marg_no_pruning=1)
    full = mcmc.DeviceBlockRunner(eng).run(start, eng.logpost(start), np.arange(2), _free(1), _chol(1, 0.3), 9, 0, 6)
    eng.set_tuning()
    assert full[4] == dev[4]
    np.testing.assert_array_equal(full[2], dev[2])
    np.testing.assert_allclose(full[3], dev[3], rtol=1e-12)
    eng.close()
