"""b9_wd_moments (the wdSummary counterpart) on the GPU: parity with the numpy statement of the definition
(tests/wdmoments_ref.py, through the comparator of tests/wdmoments_check.py), ties to b9_star_moments and b9_sample_wd_mass
on the same rows, bit-for-bit invariances, the edges of the shapes, sampler blocks left alone, the statistics of the device's
own draws against the table, and the CLI loop.  Each test makes its own short-lived engine."""

import numpy as np
import pytest

import moments_ref
import wdmoments_check as wc
import wdmoments_ref as wr
from base_amd import abi, synth
from conftest import build_problem
from cli_util import cli as _cli, read_phot as _read_phot

pytestmark = pytest.mark.gpu


class engine_for:
    """with engine_for(pack_d, cl, priors, ...) as eng: a short-lived engine on the dicts of a problem."""

    def __init__(self, pack_d, cl, priors, n_pops=1, K=1, n_q=1):
        self.args = (abi.make_pack(pack_d), abi.make_stars(cl), priors, wc.opts(n_pops, K, n_q))

    def __enter__(self):
        from base_amd import engine
        self.eng = engine.Engine(*self.args)
        return self.eng

    def __exit__(self, *exc):
        self.eng.close()


def outside(pack_d, row):
    out = np.array(row, dtype=np.float64)
    out[abi.P_LOGAGE] = pack_d["log_age"][-1] + 1.0
    return out


def against_reference(pack_d, cl, priors, n_pops, n_nodes, rows, what=""):
    """One call over `rows` against the reference's rows added up; returns (acc, x, floor)."""
    x, floor = wc.reference(pack_d, cl, rows, n_pops, n_nodes)
    with engine_for(pack_d, cl, priors, n_pops) as eng:
        acc, idx = eng.wd_moments(rows, n_nodes)
    assert np.array_equal(idx, wr.wd_stars(cl)) and acc.shape == (len(idx), 16)
    wc.assert_accumulated(acc, x, floor, what)
    return acc, x, floor


# ---- 1. parity with the reference --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["parsec", "dsed", "girardi"])
def test_parity_with_the_reference(key):
    pack_d, cl, priors, rows, n_pops, n_nodes, x, floor, amp = wc.parity_fixture(key)
    assert np.all(amp >= 0) and amp.max() <= wc.A_MAX and np.all(x[..., wr.ROWS] == 1)      # the fixture's conditions: no pair is left out
    with engine_for(pack_d, cl, priors, n_pops) as eng:
        for r in range(len(rows)):                                       # per row: one call per row, from zeros
            acc, idx = eng.wd_moments(rows[r], n_nodes)
            wc.assert_close(acc, x[r], floor[r], f"row {r}")
        assert np.array_equal(idx, np.arange(150))
        none, _ = eng.wd_moments(outside(pack_d, rows[0]), n_nodes)       # a row outside the grid adds nothing, ROWS included
        assert np.all(none == 0)
        both, _ = eng.wd_moments(np.stack([rows[2], outside(pack_d, rows[0])]), n_nodes)
        assert np.array_equal(both, eng.wd_moments(rows[2], n_nodes)[0])
        total, _ = eng.wd_moments(np.concatenate([rows, outside(pack_d, rows[0])[None]]), n_nodes)      # summed
    wc.assert_accumulated(total, x, floor, "summed")
    assert np.all(total[:, wr.ROWS] == 6)


# ---- 2. ties to existing calls on the same rows ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3])
def test_ties_to_star_moments(K):
    """At n_nodes = 8 K the grid is b9_star_moments' for a WD-stage star.  Another order of summation: not the same bits."""
    pack_d, cl, _, _, priors, _ = build_problem("dsed", 5, n_stars=300, wd_frac=0.1, n_y=3, n_pops=2, seed=12)
    rows = wc.rows_for(cl, 5, 3, 2)
    with engine_for(pack_d, cl, priors, 2, K, 2) as eng:
        mom = eng.star_moments(rows)
        acc, idx = eng.wd_moments(rows, 8 * K)
    assert len(idx) == 30 and np.all(acc[:, wr.ROWS] == 5)
    mine = acc[:, [wr.ROWS, wr.MEMBER, wr.M1, wr.M1SQ, wr.POP1]]
    theirs = mom[idx][:, [abi.MOM_ROWS, abi.MOM_MEMBER, abi.MOM_M1, abi.MOM_M1SQ, abi.MOM_POP1]]
    print("largest relative difference per column:", np.max(np.abs(mine - theirs) / np.maximum(np.abs(theirs), 1e-300), axis=0))
    np.testing.assert_allclose(mine, theirs, rtol=wc.TIE_RTOL, atol=0)
    assert np.any(acc[:, wr.POP1] > 0)


def test_ties_to_sample_wd_mass():
    pack_d, cl, priors = wc.wd_problem("parsec", 8, 400)
    rows = wc.rows_for(cl, 3, 8, 1)
    der = ("wd_mass", "prec_log_age", "log_cool_age", "log_teff", "logg")
    with engine_for(pack_d, cl, priors) as eng:
        g = eng.sample_wd_mass(rows, 512, seed=5)
        one = eng.sample_wd_mass(rows, 1, seed=5)
        for r in range(len(rows)):
            acc, _ = eng.wd_moments(rows[r], 512)
            np.testing.assert_allclose(acc[:, wr.MEMBER], g["member"][r], rtol=1e-12, atol=0)
            assert np.array_equal(acc[:, wr.ROWS], (g["zams"][r] > 0).astype(float))
            # n_nodes = 1: the increments are p (zams, zams^2, v, v^2) of the only possible draw
            acc, _ = eng.wd_moments(rows[r], 1)
            p, m = one["member"][r], one["zams"][r]
            cooled = one["log_teff"][r] != 0
            want = np.zeros_like(acc)
            want[:, wr.ROWS], want[:, wr.MEMBER], want[:, wr.COOLED] = (m > 0), p, np.where(cooled, p, 0.0)
            want[:, wr.M1], want[:, wr.M1SQ] = p * m, p * m ** 2
            for q, k in enumerate(der):
                v = np.where(cooled, one[k][r], 0.0)
                want[:, wr.WDMASS + 2 * q], want[:, wr.WDMASS + 2 * q + 1] = p * v, p * v ** 2
            np.testing.assert_allclose(acc, want, rtol=1e-14, atol=0)
            assert np.all(m > 0) and cooled.any()


# ---- 3. invariances, bit for bit -----------------------------------------------------------------------------------------------
def test_invariances_rows_calls_and_chunks():
    pack_d, cl, priors = wc.wd_problem("parsec", 8, 400)
    rows = wc.rows_for(cl, 40, 8, 1)
    with engine_for(pack_d, cl, priors) as eng:
        a, _ = eng.wd_moments(rows, 512)
        b, _ = eng.wd_moments(rows[7:], 512, acc=eng.wd_moments(rows[:7], 512)[0])           # 7 + 33
        assert np.array_equal(a, b)
        c = None
        for r in range(len(rows)):                                                           # row by row
            c, _ = eng.wd_moments(rows[r], 512, acc=c)
        assert np.array_equal(a, c)
        assert np.array_equal(a, eng.wd_moments(rows, 512)[0])                               # a repeated call
        assert np.all(a[:, wr.ROWS] == 40) and (a[:, wr.MEMBER] > 0).sum() >= 90      # (a star or two are field stars to every row)
        # a grid too fine for 12 rows' tables at once is worked in smaller chunks of rows: same bits as row by row
        fine, _ = eng.wd_moments(rows[:12], 40000)
        d = None
        for r in range(12):
            d, _ = eng.wd_moments(rows[r], 40000, acc=d)
        assert np.array_equal(fine, d)


def test_a_star_sums_the_same_whatever_shares_its_wave():
    pack_d, cl, priors = wc.wd_problem("parsec", 8, 400, keep=65)
    rows = wc.rows_for(cl, 3, 8, 1)
    res = []
    for n in (65, 64, 1):                      # star 0 in a full wave with a second wave behind it, in one wave, alone
        with engine_for(pack_d, wc.subset(cl, np.arange(n)), priors) as eng:
            res.append(eng.wd_moments(rows, 100)[0])
    assert np.array_equal(res[0][:64], res[1]) and np.array_equal(res[0][:1], res[2])
    assert res[2][0, wr.ROWS] == 3 and res[2][0, wr.M1] > 0


def test_a_permuted_catalogue_gives_the_permuted_rows():
    """Nothing here is keyed by the star's index: the accumulators follow the stars, bit for bit."""
    pack_d, cl, _, _, priors, _ = build_problem("parsec", 8, n_stars=300, wd_frac=0.2, seed=12)
    rows = wc.rows_for(cl, 4, 8, 1)
    with engine_for(pack_d, cl, priors) as eng:
        a, a_idx = eng.wd_moments(rows, 128)
    perm = np.random.default_rng(1).permutation(300)
    with engine_for(pack_d, wc.subset(cl, perm), priors) as eng:
        b, b_idx = eng.wd_moments(rows, 128)
    # star perm[j] of the first catalogue is star j of the second
    assert np.array_equal(np.sort(perm[b_idx]), a_idx) and len(a_idx) >= 40
    col = {s: j for j, s in enumerate(a_idx)}
    assert np.array_equal(b, a[[col[perm[s]] for s in b_idx]])
    assert not np.array_equal(b, a)


# ---- 4. edges of the shapes, each against the reference ----------------------------------------------------------------------------
@pytest.mark.parametrize("n_wd", [1, 63, 64, 65])
def test_star_counts_around_a_wave(n_wd):
    pack_d, cl, priors = wc.wd_problem("parsec", 8, 400, keep=n_wd)
    assert len(cl["mass1"]) == n_wd
    against_reference(pack_d, cl, priors, 1, 64, wc.rows_for(cl, 3, 8, 1))


@pytest.mark.parametrize("n_nodes", [1, 63, 64, 65, 1000])
def test_node_counts_around_a_tile(n_nodes):
    pack_d, cl, priors = wc.wd_problem("parsec", 8, 400, keep=20)
    acc, x, _ = against_reference(pack_d, cl, priors, 1, n_nodes, wc.rows_for(cl, 3, 8, 1))
    assert np.all(acc[:, wr.ROWS] == 3)


@pytest.mark.parametrize("n_pops", [1, 2])
@pytest.mark.parametrize("n_filt", [1, 4, 5, 9, 16])
def test_every_instance(n_filt, n_pops):
    pack_d, cl, priors = wc.wd_problem("dsed", n_filt, 400, n_y=3 if n_pops == 2 else 1, n_pops=n_pops, keep=40)
    assert len(cl["mass1"]) == 40
    rows = wc.rows_for(cl, 3, 3, n_pops)
    if n_pops == 2:
        rows[:, abi.P_LAMBDA] = [0.3, 0.6, 0.8]
    acc, x, _ = against_reference(pack_d, cl, priors, n_pops, 64, rows)
    assert np.all(acc[:, wr.ROWS] == 3) and (n_pops == 1 or np.any(acc[:, wr.POP1] > 0))


def test_pack_without_wd_tables():
    """Every node is without flux (a finite, hopeless chi-square) and none is cooled: COOLED and the derived sums are exactly
    0, the rest follows the reference."""
    pack_d, cl, priors = wc.wd_problem("parsec", 4, 200, keep=30)
    empty = np.zeros(0)
    pack_d = dict(pack_d, wc_carb=empty, wc_mass=empty, wc_log_age=empty, wc_log_teff=empty, wc_log_radius=empty,
                  at_logg=empty, at_log_teff=empty, at_mags=empty, n_at_type=0)
    pack_d.pop("wc_n_age", None); pack_d.pop("wc_offset", None)
    acc, x, _ = against_reference(pack_d, cl, priors, 1, 64, wc.rows_for(cl, 3, 1, 1))
    assert np.all(acc[:, wr.COOLED] == 0) and np.all(acc[:, wr.WDMASS:] == 0)
    assert np.all(acc[:, wr.ROWS] == 3) and np.all(acc[:, wr.M1] >= 0)


def test_row_whose_agb_tip_is_not_below_m_wd_up_gives_zeros():
    pack_d, cl, priors = wc.wd_problem("parsec", 4, 200, keep=30)
    rows = wc.rows_for(cl, 2, 1, 1)
    pack_d = dict(pack_d, m_wd_up=0.5)                  # below every AGB tip
    with engine_for(pack_d, cl, priors) as eng:
        assert eng.derive_isochrone(rows[0])[3] > 0.5
        acc, _ = eng.wd_moments(rows, 64)
    assert np.all(acc == 0)


def test_no_wd_stage_stars_and_invalid_arguments():
    from base_amd import engine
    pack_d, cl, _, _, priors, _ = build_problem("parsec", 4, n_stars=50, wd_frac=0.0, seed=4)
    with engine_for(pack_d, cl, priors) as eng:
        assert eng.n_wd_stars() == 0
        acc, idx = eng.wd_moments(wc.rows_for(cl, 2, 1, 1), 64)           # B9_OK, an empty result
        assert acc.shape == (0, 16) and idx.size == 0
    pack_d, cl, priors = wc.wd_problem("parsec", 4, 200, keep=3)
    rows = wc.rows_for(cl, 2, 1, 1)
    dp = abi._dp
    with engine_for(pack_d, cl, priors) as eng:
        for n_nodes in (0, -5):
            with pytest.raises(engine.B9Error) as e:
                eng.wd_moments(rows, n_nodes)
            assert e.value.code == abi.B9_ERR_INVALID
        acc = np.zeros((3, 16))
        p_rows, p_acc = rows.ctypes.data_as(dp), acc.ctypes.data_as(dp)
        assert eng.lib.b9_wd_moments(eng._ctx, p_rows, 0, 64, 0, p_acc) == abi.B9_ERR_INVALID        # n_rows < 1
        assert eng.lib.b9_wd_moments(eng._ctx, None, 2, 64, 0, p_acc) == abi.B9_ERR_INVALID
        assert eng.lib.b9_wd_moments(eng._ctx, p_rows, 2, 64, 0, None) == abi.B9_ERR_INVALID
        assert eng.lib.b9_wd_moments(None, p_rows, 2, 64, 0, p_acc) == abi.B9_ERR_INVALID
        assert np.all(acc == 0)
        assert eng.lib.b9_wd_moments(eng._ctx, p_rows, 2, 64, 0, p_acc) == abi.B9_OK and np.all(acc[:, 0] == 2)


def test_a_star_with_every_filter_unused_is_weighted_by_the_prior():
    pack_d, cl, priors = wc.wd_problem("parsec", 4, 200, keep=8)
    cl["sigma"] = np.array(cl["sigma"], dtype=np.float64)
    cl["sigma"][2] = -1.0
    rows = wc.rows_for(cl, 3, 1, 1)
    acc, x, _ = against_reference(pack_d, cl, priors, 1, 64, rows)
    tab = wr.table(acc)
    assert acc[2, wr.ROWS] == 3 and tab[2, 4] > 0.5                       # the prior over (tip, M_wd_up]: a wide posterior
    assert np.all(np.delete(tab[:, 4], 2) < tab[2, 4])


def test_cooled_weight_strictly_between_zero_and_member():
    """The seam fixture (pack A of tests/wd_seams.py: nodes above the tip whose precursor is not dead yet): the status that
    travels with the table decides which nodes enter the derived sums."""
    pack_d, cl, priors, rows, n_nodes = wc.seam_fixture()
    acc, x, _ = against_reference(pack_d, cl, priors, 1, n_nodes, rows)
    share = acc[:, wr.COOLED] / acc[:, wr.MEMBER]
    print("cooled share of the membership weight:", share)
    assert np.sum((share > 0.01) & (share < 0.99)) >= 3


# ---- 5. sampler blocks untouched, and no dependence on the context's history ----------------------------------------------------
def test_sampler_blocks_are_untouched():
    from base_amd import engine, mcmc
    pack_d, cl, pack, stars, priors, options = build_problem("parsec", 8, n_stars=400, wd_frac=0.1, seed=4)
    free = np.array(mcmc.DEFAULT_FREE)
    chol = np.diag([mcmc.DEFAULT_STEP[k] for k in free]) * 0.3
    start = synth.walker_params(cl["truth"], 4, seed=2, scale=0.3)
    rows = wc.rows_for(cl, 3, 1, 1)

    def run(interleave):
        eng = engine.Engine(pack, stars, priors, options)
        try:
            lp0 = eng.logpost(start)
            h = eng.mcmc_submit(start, lp0, np.arange(4), free, chol, 11, 0, 6, asynchronous=True)
            if interleave:
                with pytest.raises(engine.B9Error) as e:                   # B9_ERR_STATE: a block is outstanding
                    eng.wd_moments(rows, 64)
                assert e.value.code == abi.B9_ERR_STATE and "outstanding" in str(e.value)
            first = [np.array(x) for x in eng.mcmc_collect(h)[:4]]
            if interleave:
                acc, _ = eng.wd_moments(rows, 64)
                assert np.all(acc[:, wr.ROWS] == 3)
            h = eng.mcmc_submit(start, lp0, np.arange(4), free, chol, 11, 6, 6, cont=True, asynchronous=True)
            second = [np.array(x) for x in eng.mcmc_collect(h)[:4]]
        finally:
            eng.close()
        return first + second

    for a, b in zip(run(False), run(True)):
        assert np.array_equal(a, b)


def test_the_result_does_not_depend_on_the_contexts_history():
    from base_amd import engine
    pack_d, cl, pack, stars, priors, _ = build_problem("parsec", 8, n_stars=300, wd_frac=0.2, seed=12)
    rows = wc.rows_for(cl, 5, 8, 1)
    options = wc.opts(1, 2, 2)
    eng = engine.Engine(pack, stars, priors, options)
    try:
        fresh, _ = eng.wd_moments(rows, 200)
    finally:
        eng.close()
    other = wc.subset(cl, np.arange(120))
    eng = engine.Engine(pack, abi.make_stars(other), priors, options)
    try:
        eng.logpost(rows)
        eng.sample_mass(rows[:2], seed=3)
        eng.star_moments(rows)
        eng.sample_wd_mass(rows, 900, seed=2)
        eng.wd_moments(rows[:2], 77)
        eng.load_stars(stars)                                            # a reload of the stars
        used, _ = eng.wd_moments(rows, 200)
    finally:
        eng.close()
    assert np.array_equal(fresh, used) and np.all(fresh[:, wr.ROWS] == 5)


# ---- 6. statistics against the device's draws -----------------------------------------------------------------------------------
def test_statistics_against_device_draws():
    """One star, one row repeated 4000 times: the means of the device's draws against the table's means, with the reference's
    variances.  The test's power: the second-moment mutant's table fails it."""
    pack_d, cl, priors, rows = wc.stat_problem()
    with engine_for(pack_d, cl, priors) as eng:
        g = eng.sample_wd_mass(rows, wc.STAT_NODES, seed=wc.STAT_SEED)
        acc, _ = eng.wd_moments(rows[0], wc.STAT_NODES)
    from base_amd import engine
    z = wc.stat_z(pack_d, cl, rows, g, engine.wd_table(acc))
    print("|z| of the mean drawn zams, wd_mass, log_cool_age:", np.abs(z))
    assert len(z) == 3 and np.all(np.abs(z) <= moments_ref.Z_MAX)
    mutant = wr.table(wr.accumulate(pack_d, cl, rows[:1], 1, wc.STAT_NODES, second_moment_power=1))
    assert not np.all(np.abs(wc.stat_z(pack_d, cl, rows, g, mutant)) <= moments_ref.Z_MAX)


# ---- 7. the CLI loop --------------------------------------------------------------------------------------------------------------
def test_cli_loop_file_equals_the_engine_and_agrees_with_the_draws(tmp_path):
    """simCluster (seeded, WD primaries) -> scatterCluster -> singlePopMcmc (short) -> wdSummary, and sampleWDMass on the same
    chain.  Every step runs under its own time limit and a failed step ends the test."""
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
    r = _cli("wdSummary", "--config", y, "--nMassNodes", str(n_nodes))
    assert r.returncode == 0, r.stderr
    assert "node evaluations/s" in r.stderr and "%d mass nodes" % n_nodes in r.stderr
    r = _cli("sampleWDMass", "--config", y, "--nMassNodes", str(n_nodes), "--seed", "31")
    assert r.returncode == 0, r.stderr

    # the file parses; its ids are the stage-3 stars in .phot order
    cl = _read_phot(base + ".sim.scatter")
    ids = [ln.split()[0] for ln in open(base + ".sim.scatter").read().splitlines()[1:]]
    wd = np.flatnonzero(cl["stage"] == abi.STAGE_WD)
    assert len(wd) >= 100
    got_ids, cols, tab = hostlib.read_wd_summary(fit + ".wdSummary")
    assert cols == list(hostlib.WD_TABLE_COLUMNS[:15]) and got_ids == [ids[i] for i in wd]
    rows = hostlib.read_res_rows(fit + ".res", start, 3)
    assert len(rows) == 300 * 4
    eng = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cl), synth.default_priors(pack_d, truth), wc.opts())
    try:
        acc, idx = eng.wd_moments(rows, n_nodes)
        tip = eng.derive_isochrone(truth)[3]
    finally:
        eng.close()
    assert np.array_equal(idx, wd)
    np.testing.assert_allclose(tab, engine.wd_table(acc)[:, :15], rtol=0, atol=6e-7)             # %.6f
    assert np.all(tab[:, 0] == len(rows))

    # against the draws of the same chain: zamsMass inside the 0.5 % .. 99.5 % quantiles of the star's sampleWDMass draws,
    # widened by one node spacing, for at least 90 % of the stars with member >= 0.5
    zams = np.loadtxt(fit + ".wd.zamsMass", skiprows=1, ndmin=2)
    assert zams.shape == (len(rows), len(wd))
    spacing = (pack_d["m_wd_up"] - tip) / n_nodes
    lo, hi = np.quantile(zams, [0.005, 0.995], axis=0)
    member = tab[:, 1] >= 0.5
    inside = (tab[:, 3] >= lo - spacing) & (tab[:, 3] <= hi + spacing)
    print(f"{inside[member].mean():.1%} of {int(member.sum())} WD-stage stars with member >= 0.5 have zamsMass inside the 99 % interval of "
          f"their draws (node spacing {spacing:.4f} Msun)")
    assert member.sum() >= 50 and inside[member].mean() >= 0.9

    # a catalogue without WD-stage stars is an error with a clear message; so is --nMassNodes 0
    r = _cli("simCluster", "--config", y_true, "--nStars", "60", "--minMass", "0.6", "--maxMass", "1.0")
    assert r.returncode == 0, r.stderr
    r = _cli("scatterCluster", "--config", y_true, "--sigmaFloor", "0.01", "--sigmaAtLimit", "0.05", "--faintLimit", "45")
    assert r.returncode == 0, r.stderr
    r = _cli("wdSummary", "--config", y, "--nMassNodes", str(n_nodes))
    assert r.returncode != 0 and "no WD-stage star" in r.stderr
    r = _cli("wdSummary", "--config", y, "--nMassNodes", "0")
    assert r.returncode != 0
