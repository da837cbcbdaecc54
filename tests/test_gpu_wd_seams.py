"""The WD branch at its seams on the device, against the 50-digit reference (tests/wd_ref.py) at the cases of
tests/wd_seams.py.  Tolerance everywhere: 2 x the reference's own error budget + 1 ulp of the value.

  R1  the general form (star_mags -> wd_chain -> wd_atmosphere): b9_predict_mags
  R2  the lean form (comp_desc / comp_mag, the heavy role of k_star_like): b9_logpost, given-mass, per star -- the seam stars
      alone, scattered among 200 MS stars, and under two populations
  R3  the two forms against each other: the lean form's chi^2 at the general form's magnitudes must be exactly 0
  R4  the sampler's heavy role (k_mcmc_tree with 1 walker, k_mcmc_step with 8) on the mixed catalogue
  R5  the marginalised tables: WD-stage stars' per-star values (k_marg_wd_table / k_star_marg_wd, and k_marg_step's own table
      builder through a short block) against the reference's sum over the nodes tip + j dM; b9_sample_wd_mass's five derived
      values (k_wd_node_table) at the drawn mass
and the device library's exp10 / log10 over the chain's argument range against mpmath (the budget's 3 ulp).
Only families d (cancellation) and NaN are compared weakly: within the budget, however large, and finite unless the reference
is not.  Each test prints the largest |device - reference| / tolerance per family (docs/LABNOTES.md records them)."""
import math

import numpy as np
import pytest

import oracle
import wd_ref as R
import wd_seams as S
from base_amd import abi, synth

pytestmark = pytest.mark.gpu
PACKS = ["A", "Aw", "As", "Ap", "Al", "B", "C", "D"]
SIGMA, PRIOR = 0.03125, 0.875
_ENG = {}


def _engine(name):
    from base_amd import engine
    if name not in _ENG:
        _ENG[name] = engine.Engine(abi.make_pack(S.packs()[name][0]))
        _ENG[name].set_priors(abi.make_priors())
    return _ENG[name]


def _report(route, name, worst, n_weak):
    print(f"\n{route} pack {name}: max |device - reference| / tolerance per family "
          f"{ {k: float(f'{v:.3g}') for k, v in sorted(worst.items())} }; {n_weak} weak cases (families d, NaN)")


def _by_row(name, single_only=False, with_dne=True):
    out = {}
    for c in S.cases():
        if c["pack"] == name and (with_dne or c["m1"] > 0.0) and not (single_only and c["q"] > 0.0):
            out.setdefault(c["row"], []).append(c)
    return out


def _predict(name, irow, cs):
    d, rows = S.packs()[name]
    return _engine(name).predict_mags(rows[irow], [c["m1"] for c in cs], [c["q"] for c in cs], [c["wd_type"] for c in cs])


@pytest.mark.parametrize("name", PACKS)
def test_r1_general_form_predict_mags(name):
    d, rows = S.packs()[name]
    worst, n_weak = {}, 0
    for irow, cs in _by_row(name).items():
        assert len(cs) <= 400
        mags, stage = _predict(name, irow, cs)
        tip = float(S.model(name, irow).tip.v)
        for c, g, st in zip(cs, mags, stage):
            want = abi.STAGE_MSRG if c["m1"] <= tip else (abi.STAGE_WD if c["m1"] <= d["m_wd_up"] else abi.STAGE_NSBH)
            assert st == want, (c["fam"], irow, c["m1"], st, want)
            r = S.mag_ratio(c, g)
            assert c["fam"] in S.WEAK or S.meets_budget(c["ref"])
            assert r <= 1.0, (c["fam"], name, irow, c["m1"], c["q"], c["wd_type"], r, list(g))
            worst[c["fam"]] = max(worst.get(c["fam"], 0.0), r)
            n_weak += c["fam"] in S.WEAK
    _report("R1", name, worst, n_weak)


def _check_values(name, cs, got, sigma, prior, worst, key="value"):
    n_weak = 0
    for c, g in zip(cs, got):
        want = S.like(name, c, sigma, prior)[key if c["fam"] != "NaN" else "value"]
        r = S.value_ratio(want, g)
        assert r <= 1.0, (c["fam"], name, c["row"], c["m1"], c["q"], c["wd_type"], g, want and float(want.v), r)
        assert not math.isnan(g)
        worst[c["fam"]] = max(worst.get(c["fam"], 0.0), r)
        n_weak += c["fam"] in S.WEAK
    return n_weak


@pytest.mark.parametrize("name", PACKS)
def test_r2_lean_form_logpost_alone(name):
    d, rows = S.packs()[name]
    eng = _engine(name)
    eng.set_options(abi.make_options())
    worst, n_weak = {}, 0
    for irow, (cl, cs) in S.catalogue(name, prior=PRIOR, sigma=SIGMA).items():
        eng.load_stars(abi.make_stars(cl))
        tot, ps = eng.logpost(rows[irow][None, :], perstar=True)
        assert math.isfinite(tot[0])
        n_weak += _check_values(name, cs, ps[0], SIGMA, PRIOR, worst)
    _report("R2 (alone)", name, worst, n_weak)


def _fillers(d, row, n, seed):
    """n MS stars (half of them binaries) observed at the numpy forward model's magnitudes + the known offsets"""
    rng = np.random.default_rng(seed)
    _, imass, _ = synth.derive_isochrone(d, row[abi.P_LOGAGE], row[abi.P_FEH], row[abi.P_Y])
    m = rng.uniform(imass[0] * 1.01, imass[-1] * 0.99, n)
    q = np.where(np.arange(n) % 2 == 0, 0.0, rng.uniform(0.2, 0.95, n))
    obs = synth.forward_mags(d, row, m, q) + S.OFFSETS[:d["n_filt"]][None, :]
    return m, q, obs


@pytest.mark.parametrize("name", ["A", "Al", "B", "C"])
def test_r2_lean_form_scattered_among_ms_stars(name):
    """the heavy role shares its kernel with the hot role: the same seam stars, scattered among 200 MS stars"""
    d, rows = S.packs()[name]
    eng = _engine(name)
    eng.set_options(abi.make_options())
    worst, n_weak = {}, 0
    for irow, (cl, cs) in S.catalogue(name, prior=PRIOR, sigma=SIGMA).items():
        m, q, obs = _fillers(d, rows[irow], 200, 100 + irow)
        n = len(cs) + 200
        where = np.sort(np.random.default_rng(irow).permutation(n)[:len(cs)])
        mixed = {k: (np.zeros((n,) + np.asarray(v).shape[1:], dtype=np.asarray(v).dtype) if k in
                     ("obs", "sigma", "mass1", "mass_ratio", "clust_prior", "stage", "wd_type") else v) for k, v in cl.items()}
        rest = np.setdiff1d(np.arange(n), where)
        for k in ("obs", "sigma", "mass1", "mass_ratio", "clust_prior", "stage", "wd_type"):
            mixed[k][where] = cl[k]
        mixed["obs"][rest], mixed["mass1"][rest], mixed["mass_ratio"][rest] = obs, m, q
        mixed["sigma"][rest], mixed["clust_prior"][rest], mixed["stage"][rest] = SIGMA, PRIOR, abi.STAGE_MSRG
        stars = abi.make_stars(mixed)
        eng.load_stars(stars)
        tot, ps = eng.logpost(rows[irow][None, :], perstar=True)
        n_weak += _check_values(name, cs, ps[0][where], SIGMA, PRIOR, worst)
        want = oracle.Oracle(abi.make_pack(d), stars, abi.make_priors(), abi.make_options()).logpost(rows[irow][None, :], perstar=True)
        assert np.max(np.abs(ps[0][rest] - want[1][0][rest]) / np.maximum(1.0, np.abs(want[1][0][rest]))) <= 1e-9
        # (not against the oracle's total: the stars of the weak families may differ from it by their budget, which is large)
        assert math.isfinite(tot[0]) and abs(tot[0] - ps[0].sum()) <= 1e-9 * max(1.0, abs(tot[0]))
    _report("R2 (scattered)", name, worst, n_weak)


def test_r2_lean_form_two_populations():
    """pack B (n_y = 3), two populations: log(lambda L_A + (1 - lambda) L_B) of the reference's two log-likelihoods"""
    name = "B"
    d, rows = S.packs()[name]
    eng = _engine(name)
    eng.set_options(abi.make_options(n_pops=2))
    worst, n_weak = {}, 0
    M = R.M
    try:
        for irow, (cl, cs) in S.catalogue(name, prior=PRIOR, sigma=SIGMA).items():
            eng.load_stars(abi.make_stars(cl))
            tot, ps = eng.logpost(rows[irow][None, :], perstar=True)
            assert math.isfinite(tot[0])
            lam, nf = M.mpf(float(rows[irow][abi.P_LAMBDA])), d["n_filt"]
            fld = M.ln(1 - M.mpf(PRIOR)) + M.mpf(S.LOG_FS(nf))
            for c, g in zip(cs, ps[0]):
                obs, sig = S.case_obs(d, rows[irow], c), np.full(nf, SIGMA)
                lls = [R.loglike(R.REF, d, R.evaluate(d, rows[irow], k, c["m1"], c["q"], c["wd_type"], model=S.model(name, irow, k)),
                                 c["m1"], obs, sig, 1.0, None)["ll"] for k in (0, 1)]
                terms = [(w + x.v, x.e) for w, x in zip((M.ln(lam), M.ln(1 - lam)), lls) if x is not None]
                terms = [(M.ln(M.mpf(PRIOR)) + v, e) for v, e in terms] + [(fld, 0)]
                top = max(v for v, _ in terms)
                v = top + M.ln(sum(M.exp(t - top) for t, _ in terms))
                e = sum(M.exp(t - v) * e for t, e in terms) + 2 * M.mpf("4e-16") + 16 * R.U * (1 + abs(v) + abs(M.ln(lam)) + abs(M.ln(1 - lam)))
                r = S.value_ratio(R.V(v, e), g)
                assert r <= 1.0, (c["fam"], irow, c["m1"], c["q"], g, float(v), r)
                worst[c["fam"]] = max(worst.get(c["fam"], 0.0), r)
                n_weak += c["fam"] in S.WEAK
    finally:
        eng.set_options(abi.make_options())
    _report("R2 (two populations)", name, worst, n_weak)


@pytest.mark.parametrize("name", PACKS)
def test_r3_lean_form_at_the_general_forms_magnitudes(name):
    """obs = b9_predict_mags' output, sigma = 2^-40, membership prior 1: the per-star value is c0 (mass prior + Gaussian
    constants) to 1e-12 relative only if the lean form (comp_desc / comp_mag, bracket8, fdiv, prec_corners) forms the SAME BITS
    as the general one -- one ulp of a magnitude of 10 in one filter moves it by 1e-8.  Single stars that give flux, outside the
    NaN family (a system without flux is B9_MAG_NOFLUX to b9_predict_mags but B9_MAG_NOFLUX + modulus to the likelihood).  The
    NaN family rides along at prior 1: its stars are impossible (-inf) and the total is -inf, never NaN."""
    d, rows = S.packs()[name]
    eng = _engine(name)
    eng.set_options(abi.make_options())
    sig = 2.0 ** -40
    worst, n = 0.0, 0
    for irow, cs in _by_row(name, single_only=True, with_dne=False).items():
        cs = [c for c in cs if "system:no_flux" not in c["ref"]["tags"]]
        if not cs:
            continue
        mags, _ = _predict(name, irow, cs)
        nan = np.array([c["fam"] == "NaN" for c in cs])
        assert not np.isfinite(mags[nan]).any() and np.isfinite(mags[~nan]).all()
        cl = S.cluster_of(d, cs, np.where(np.isfinite(mags), mags, 20.0), sig, 1.0)
        eng.load_stars(abi.make_stars(cl))
        tot, ps = eng.logpost(rows[irow][None, :], perstar=True)
        assert not math.isnan(tot[0]) and (tot[0] == -math.inf if nan.any() else math.isfinite(tot[0]))
        k = int(np.flatnonzero(~nan)[0])           # the comparison has the power it claims: one ulp in one magnitude shows
        f = int(np.argmax(np.abs(cl["obs"][k])))    # (its largest magnitude: one ulp of a magnitude below 1/8 would be too small to see)
        assert abs(cl["obs"][k, f]) >= 1.0
        cl["obs"][k, f] = math.nextafter(cl["obs"][k, f], math.inf)
        eng.load_stars(abi.make_stars(cl))
        moved = eng.logpost(rows[irow][None, :], perstar=True)[1][0][k]
        assert abs(moved - ps[0][k]) > 1e-10 * abs(ps[0][k]), (moved, ps[0][k])
        for c, g in zip(cs, ps[0]):
            if c["fam"] == "NaN":
                assert g == -math.inf
                continue
            c0 = float(S.like(name, c, sig, 1.0)["c0"].v)
            r = abs(g - c0) / abs(c0)
            assert r <= 1e-12, (c["fam"], name, irow, c["m1"], c["wd_type"], g, c0, r)
            worst, n = max(worst, r), n + 1
    print(f"\nR3 pack {name}: {n} single stars, max |value - c0| / |c0| = {worst:.3g} (a one-ulp disagreement would give ~1e-8)")


@pytest.mark.parametrize("walkers", [1, 8])
def test_r4_sampler_heavy_role(walkers):
    """A short block on the mixed catalogue of pack Al (linear IFMR; its intercept, slope and the carbonicity are sampled), the
    walkers started next to rows of families c (the not-yet-dead band), e (wd_mass below, on and above the axis, tiny, <= 0) and f
    (carbonicity outside its axis): every recorded log-posterior equals b9_logpost at the recorded position to 1e-9 relative,
    the tolerance tests/test_gpu_sampler.py uses for this comparison."""
    name = "Al"
    d, rows = S.packs()[name]
    eng = _engine(name)
    eng.set_options(abi.make_options())
    cl, cs = S.catalogue(name, prior=PRIOR, sigma=SIGMA)[0]
    m, q, obs = _fillers(d, rows[0], 200, 7)
    n = len(cs) + 200
    mixed = dict(cl)
    for k, v in (("obs", obs), ("mass1", m), ("mass_ratio", q), ("sigma", np.full(obs.shape, SIGMA)), ("clust_prior", np.full(200, PRIOR)),
                 ("stage", np.full(200, abi.STAGE_MSRG, np.int32)), ("wd_type", np.zeros(200, np.int32))):
        mixed[k] = np.concatenate([np.asarray(cl[k]), v])
    eng.load_stars(abi.make_stars(mixed))
    start = np.array([rows[i % 7] for i in range(walkers)])
    start[:, abi.P_CARBONICITY] = [(0.125, 0.5, 0.9375, 0.375)[i % 4] for i in range(walkers)]
    free = np.array([abi.P_LOGAGE, abi.P_FEH, abi.P_MOD, abi.P_ABS, abi.P_CARBONICITY, abi.P_IFMR_INTERCEPT, abi.P_IFMR_SLOPE], dtype=np.int32)
    chol = np.diag([2e-5, 1e-4, 1e-3, 1e-3, 1e-3, 1e-3, 1e-3])
    lp0 = eng.logpost(start)
    assert np.all(np.isfinite(lp0))
    n_steps = 12
    _, _, samples, lps, n_acc = eng.mcmc_run_block(start, lp0, np.arange(walkers, dtype=np.int32), free, chol, 5, 0, n_steps)
    pos = np.repeat(start[None, :, :], n_steps, axis=0)
    pos[:, :, free] = samples
    want = eng.logpost(pos.reshape(-1, abi.B9_NPARAM)).reshape(n_steps, walkers)
    assert not np.isnan(lps).any()
    err = np.max(np.abs(lps - want) / np.maximum(1.0, np.abs(want)))
    print(f"\nR4 {walkers} walker(s): {n_steps * walkers} recorded log-posteriors, accepted {n_acc}, max rel. difference from b9_logpost {err:.3g}")
    assert n_acc > 0 and err <= 1e-9


@pytest.mark.parametrize("name,irows", [("A", (0, 3, 5)), ("Al", (0, 3, 4, 5, 6)), ("B", (0, 10, 12)), ("C", (0,))])
def test_r5_sample_wd_mass_derived_values(name, irows):
    """b9_sample_wd_mass (k_wd_node_table: the general form through the table kernel): the five derived values it reports at the
    drawn ZAMS mass against the reference's intermediates at that mass -- rows with the carbonicity outside its axis and with an
    IFMR that gives wd_mass <= 0 at some (Al rows 4, 5: at every node up to m = 3 resp. 5) nodes; a drawn node whose precursor
    has not died reports 0 for the last three."""
    d, rows = S.packs()[name]
    eng = _engine(name)
    eng.set_options(abi.make_options())
    cl, cs = S.catalogue(name, prior=PRIOR, sigma=SIGMA)[0]
    eng.load_stars(abi.make_stars(cl))
    n_nodes, up = 16, float(d["m_wd_up"])
    keys = ("wd_mass", "prec_log_age", "log_cool_age", "log_teff", "logg")
    worst, n_live, n_notyet = {}, 0, 0
    for seed in (1, 2):
        res = eng.sample_wd_mass(np.array([rows[i] for i in irows]), n_nodes, seed=seed)
        assert res["zams"].shape == (len(irows), len(cs))
        for ri, irow in enumerate(irows):
            md = S.model(name, irow)
            tip = float(md.tip.v)
            dM = (up - tip) / n_nodes
            for s in range(len(cs)):
                z = float(res["zams"][ri, s])
                got = [float(res[k][ri, s]) for k in keys]
                if z == 0.0:
                    assert got == [0.0] * 5 and res["member"][ri, s] == 0.0
                    continue
                j = round((z - tip) / dM)
                assert 1 <= j <= n_nodes and abs(z - (tip + dM * j)) <= 2 * math.ulp(z)
                if z > up:                          # rounding put the last node above M_wd_up: no flux, no derived values
                    assert got == [0.0] * 5
                    continue
                out = {}
                st = md.wd_chain(z, set(), out)
                assert st in (R.WD, R.WD_NOTYET)
                n_live, n_notyet = n_live + 1, n_notyet + (st == R.WD_NOTYET)
                want = [out["wd_mass"], out["prec"]] + ([out["log_cool"], out["log_teff"], out["logg"]] if st == R.WD else [None] * 3)
                for k, w, g in zip(keys, want, got):
                    if w is None:
                        assert g == 0.0, (k, irow, z, g)
                        continue
                    assert float(w.e) <= 1e-9 * max(1.0, abs(float(w.v))), "a drawn node outside the budget condition"
                    r = S.value_ratio(w, g)
                    assert r <= 1.0, (k, name, irow, z, g, float(w.v), r)
                    worst[k] = max(worst.get(k, 0.0), r)
    assert n_live > 0
    print(f"\nR5 pack {name}: {n_live} draws ({n_notyet} not yet dead), max |device - reference| / tolerance "
          f"{ {k: float(f'{v:.3g}') for k, v in worst.items()} }")


def test_r5_sample_wd_mass_without_a_mass_range():
    """dM <= 0 (M_wd_up below the AGB tip): every output is 0"""
    from base_amd import engine
    d, rows = S.packs()["C"]
    low = dict(d, m_wd_up=0.5 * float(S.model("C", 0).tip.v))
    cl, cs = S.catalogue("C", prior=PRIOR, sigma=SIGMA)[0]
    eng = engine.Engine(abi.make_pack(low), abi.make_stars(cl), abi.make_priors(), abi.make_options())
    res = eng.sample_wd_mass(rows[0][None, :], 16, seed=3)
    for k in ("zams", "member") + eng.WD_DERIVED:
        assert np.all(res[k] == 0.0), k
    eng.close()


def _marg_reference(name, irow, cs, K, prior):
    """The reference's per-star value of WD-stage stars in the marginalised mode: log-sum-exp over the nodes m_j = tip + dM j,
    j = 1 .. 8 K, of ll(m_j) + log dM, then the field-star mixture.  The node masses are formed in fp64 exactly as
    k_marg_wd_table forms them (dM = (M_wd_up - tip) / steps; a product, then a sum) and enter the reference as exact inputs.
    A node whose magnitudes are not finite (wd_mass <= 0) does not take part; one that rounding puts above M_wd_up has no flux."""
    d, rows = S.packs()[name]
    M, nf, steps = R.M, d["n_filt"], 8 * K
    md = S.model(name, irow)
    tip, up = float(md.tip.v), float(d["m_wd_up"])
    dM = (up - tip) / steps
    nodes = {}
    if dM > 0.0:
        for j in range(1, steps + 1):
            for ty in (0, 1):
                nodes[j, ty] = R.evaluate(d, rows[irow], 0, tip + dM * j, 0.0, ty, model=md)
    out, sig = [], np.full(nf, SIGMA)
    fld = M.ln(1 - M.mpf(prior)) + M.mpf(S.LOG_FS(nf))
    for c in cs:
        obs = S.case_obs(d, rows[c["row"]], c)
        terms = []
        for j in range(1, steps + 1):
            if dM > 0.0:
                r = nodes[j, c["wd_type"]]
                ll = R.loglike(R.REF, d, r, tip + dM * j, obs, sig, 1.0, None)["ll"]
                if ll is not None:
                    assert float(ll.e) <= 1e-9 * max(1.0, abs(float(ll.v))), "a node outside the budget condition"
                    terms.append((ll.v + M.ln(M.mpf(dM)) + M.ln(M.mpf(prior)), ll.e))
        terms.append((fld, 0))
        top = max(v for v, _ in terms)
        v = top + M.ln(sum(M.exp(t - top) for t, _ in terms))
        # first order: every term's budget enters with its share exp(t - v) of the sum (a node 1e4 e-folds down contributes nothing)
        out.append(R.V(v, sum(M.exp(t - v) * e for t, e in terms) + M.mpf("4e-16") + 64 * R.U * (1 + abs(v))))
    return out


@pytest.mark.parametrize("name,irows", [("A", (0, 3, 5)), ("Al", (0, 4, 5)), ("B", (0, 10, 12)), ("C", (0,))])
def test_r5_marginalised_wd_stage_stars(name, irows):
    """b9_logpost, marginalised mode, stars of stage WD observed at the nodes' own magnitudes: the general form
    through k_marg_wd_table, at rows with the carbonicity below / above its axis and with wd_mass <= 0 at the nodes up to m = 3
    resp. 5 (pack Al rows 4, 5: those nodes are impossible and the others carry the star)."""
    d, rows = S.packs()[name]
    eng = _engine(name)
    K, worst, n = 1, 0.0, 0
    m, q, obs = _fillers(d, rows[0], 16, 3)          # 16 MS-stage stars beside them (their integral is not this test's subject)
    eng.set_options(abi.make_options(abi.MODE_MARGINALISED, 1, K, 2))
    try:
        for irow in irows:
            # one star ON every node's own magnitudes (+ the known offsets), DA and DB: the cluster term carries its value, and
            # the node beside it enters at a few e-folds below (an impossible node's star, observed at 20 mag, is carried by the rest)
            md = S.model(name, irow)
            tip = float(md.tip.v)
            dM = (float(d["m_wd_up"]) - tip) / (8 * K)
            cs = [dict(m1=tip + dM * j, q=0.0, wd_type=ty, row=irow, ref=R.evaluate(d, rows[irow], 0, tip + dM * j, 0.0, ty, model=md))
                  for j in range(1, 8 * K + 1) for ty in (0, 1)]
            cl = S.cluster_of(d, cs, np.array([S.case_obs(d, rows[irow], c) for c in cs]), SIGMA, PRIOR)
            for k, v in (("obs", obs), ("mass1", m), ("mass_ratio", q), ("sigma", np.full(obs.shape, SIGMA)), ("clust_prior", np.full(16, PRIOR)),
                         ("stage", np.full(16, abi.STAGE_MSRG, np.int32)), ("wd_type", np.zeros(16, np.int32))):
                cl[k] = np.concatenate([cl[k], v])
            eng.load_stars(abi.make_stars(cl))
            tot, ps = eng.logpost(rows[irow][None, :], perstar=True)
            assert math.isfinite(tot[0])
            fld = math.log1p(-PRIOR) + S.LOG_FS(d["n_filt"])
            for c, want, g in zip(cs, _marg_reference(name, irow, cs, K, PRIOR), ps[0]):
                r = S.value_ratio(want, g)
                assert r <= 1.0, (name, irow, c["m1"], c["wd_type"], g, float(want.v), r)
                worst, n = max(worst, r), n + (g > fld + 1.0)
        if name == "A":      # k_marg_step builds its own WD table: every log-posterior a short block records equals b9_logpost there
            start = np.array([rows[0], rows[3]])
            free = np.array([abi.P_LOGAGE, abi.P_FEH, abi.P_MOD, abi.P_ABS, abi.P_CARBONICITY], dtype=np.int32)
            chol = np.diag([2e-5, 1e-4, 1e-3, 1e-3, 1e-2])
            _, _, smp, lps, _ = eng.mcmc_run_block(start, eng.logpost(start), np.arange(2, dtype=np.int32), free, chol, 5, 0, 8)
            pos = np.repeat(start[None, :, :], 8, axis=0)
            pos[:, :, free] = smp
            want = eng.logpost(pos.reshape(-1, abi.B9_NPARAM)).reshape(8, 2)
            assert np.max(np.abs(lps - want) / np.maximum(1.0, np.abs(want))) <= 1e-9
    finally:
        eng.set_options(abi.make_options())
    assert n >= 8 * len(irows), "the cluster term must carry most stars, or the comparison only sees the field term"
    print(f"\nR5 (marginalised) pack {name}: 16 WD-stage stars x {len(irows)} rows ({n} carried by the cluster term), "
          f"max |device - reference| / tolerance {worst:.3g}")


def test_r5_marginalised_without_a_mass_range():
    """dM <= 0 (M_wd_up below the AGB tip): no node, every WD-stage star is a field star"""
    from base_amd import engine
    d, rows = S.packs()["C"]
    low = dict(d, m_wd_up=0.5 * float(S.model("C", 0).tip.v))
    cl, cs = S.catalogue("C", prior=PRIOR, sigma=SIGMA)[0]
    eng = engine.Engine(abi.make_pack(low), abi.make_stars(cl), abi.make_priors(), abi.make_options(abi.MODE_MARGINALISED, 1, 1, 2))
    tot, ps = eng.logpost(rows[0][None, :], perstar=True)
    want = math.log1p(-PRIOR) + S.LOG_FS(d["n_filt"])
    assert np.all(np.abs(ps[0] - want) <= 4 * math.ulp(want)) and math.isfinite(tot[0])
    eng.close()


def test_device_exp10_log10_over_the_chains_argument_range():
    """The library's exp10 and log10 as wd_chain calls them, over the arguments the chain can give them -- exp10 of logAge and
    prec (6.5 .. 10.5), log10 of 10^logAge - 10^prec (1 .. 3e10), of m / tips[0] (1 .. 100) and of wd_mass (1e-9 .. 40) --
    against mpmath: the budget of tests/wd_ref.py allows them 3 ulp each.  The measured maxima are printed."""
    import prims_probe
    import prims_ref as PR
    P = prims_probe.load()
    rng = np.random.default_rng(20)
    xe = np.concatenate([rng.uniform(6.5, 10.5, 3000), S.packs()["A"][0]["log_age"], S.packs()["C"][0]["log_age"]])
    xl = np.concatenate([10.0 ** rng.uniform(0.0, 10.5, 2000), rng.uniform(1.0, 100.0, 1000), 10.0 ** rng.uniform(-9.0, 1.6, 1000),
                         1.0 + rng.uniform(0.0, 1e-6, 200)])
    ge, gl = P.map1("exp10", xe), P.map1("log10", xl)
    we = [PR.ulp_error(float(g), PR.mpmath.power(10, PR.mpf(float(x)))) for g, x in zip(ge, xe)]
    wl = [PR.ulp_error(float(g), PR.mpmath.log10(PR.mpf(float(x)))) for g, x in zip(gl, xl)]
    print(f"\ndevice exp10 on [6.5, 10.5]: max {max(we):.3f} ulp; device log10 on the chain's arguments: max {max(wl):.3f} ulp")
    assert max(we) <= 3.0 and max(wl) <= 3.0
