"""b9_star_moments (the starSummary counterpart) on the GPU: every accumulator against the numpy statement
tests/moments_ref.py, the edges of the star and node shapes, the tie to b9_sample_mass, bit-for-bit invariances, the sampler
left alone, statistics against the device's own draws, every kernel instance, and the CLI.  Each test makes its own
short-lived engine on the small packs of build_problem(small=True).

Tolerance of every comparison with the reference: rtol 1e-9 -- the project's per-star tolerance --
and, because the kernel prunes, atol = N_nodes e^-40 on components 1..7 (N_nodes: the nodes of a star's grid, all
populations; stated per case)."""
import ctypes as C

import numpy as np
import pytest

import moments_ref as mr
from base_amd import abi, synth
from conftest import build_problem
from cli_util import cli as _cli, read_phot as _read_phot

pytestmark = pytest.mark.gpu

PER_STAR = ("obs", "sigma", "mass1", "mass_ratio", "clust_prior", "stage", "wd_type", "is_field", "pop")
RTOL = 1e-9


def subset(cl, sel):
    """The cluster dict reduced to the stars `sel` (mask or index array)."""
    out = dict(cl)
    for k in PER_STAR:
        out[k] = np.ascontiguousarray(np.asarray(cl[k])[sel])
    return out


def rows_for(pack_d, cl, n_pops, n_rows=3, outside=True):
    """The cases' rows: walker_params(truth, n_rows, seed 3, scale 0.3), lambda clipped, + one row outside the age grid."""
    rows = synth.walker_params(cl["truth"], n_rows, seed=3, scale=0.3)
    if n_pops == 2:
        rows[:, abi.P_LAMBDA] = np.clip(rows[:, abi.P_LAMBDA], 0.05, 0.95)
    if outside:
        out = rows[:1].copy()
        out[0, abi.P_LOGAGE] = pack_d["log_age"][-1] + 1.0
        rows = np.concatenate([rows, out])
    return rows


def opts(n_pops, K, Q, mode=abi.MODE_GIVEN_MASS):
    return abi.make_options(mode=mode, n_pops=n_pops, marg_iso_increm=K, marg_n_q=Q)


def device_moments(pack, stars, priors, n_pops, K, Q, rows):
    from base_amd import engine
    eng = engine.Engine(pack, stars, priors, opts(n_pops, K, Q))
    try:
        return eng.star_moments(rows)
    finally:
        eng.close()


def n_nodes_of(pack_d, n_pops, K, Q):
    return n_pops * max((int(np.max(pack_d["iso_n_eep"])) - 1) * K * Q, 8 * K)


def assert_close(got, want, n_nodes):
    assert np.array_equal(got[:, 0], want[:, 0])                       # ROWS is a count
    atol = n_nodes * np.exp(-40.0)
    for c in range(1, 8):
        np.testing.assert_allclose(got[:, c], want[:, c], rtol=RTOL, atol=atol, err_msg=f"component {c}")


def against_reference(pack_d, cl, pack, stars, priors, n_pops, K, Q, rows=None, n_nodes=None):
    rows = rows_for(pack_d, cl, n_pops) if rows is None else rows
    got = device_moments(pack, stars, priors, n_pops, K, Q, rows)
    want = mr.accumulate(pack_d, cl, rows, n_pops, K, Q)
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    print(f"largest relative difference per component: {np.where(want != 0, rel, 0).max(axis=0)}")
    assert_close(got, want, n_nodes or n_nodes_of(pack_d, n_pops, K, Q))
    return got, want


# ---- 1. parity with the reference -----------------------------------------------------------------------------------------
CASES = [   # pack, filters, n_y, pops, K, Q, stars, wd_frac, N_nodes = pops * 89 EEP intervals * K * Q
    ("dsed", 5, 3, 2, 2, 2, 130, 0.1, 712),
    ("parsec", 8, 1, 1, 1, 4, 130, 0.1, 356),
    ("girardi", 3, 1, 1, 3, 1, 70, 0.0, 267),
    ("parsec", 9, 1, 1, 1, 2, 70, 0.1, 178),
]


@pytest.mark.parametrize("name,n_filt,n_y,n_pops,K,Q,n_stars,wd_frac,n_nodes", CASES)
def test_parity_with_reference(name, n_filt, n_y, n_pops, K, Q, n_stars, wd_frac, n_nodes):
    pack_d, cl, pack, stars, priors, _ = build_problem(name, n_filt, n_stars=n_stars, wd_frac=wd_frac, n_y=n_y, n_pops=n_pops, seed=12)
    assert n_nodes == n_nodes_of(pack_d, n_pops, K, Q)
    got, want = against_reference(pack_d, cl, pack, stars, priors, n_pops, K, Q, n_nodes=n_nodes)
    live = want[:, mr.MEMBER] > 0
    assert np.all(got[got[:, 0] > 0, 0] == 3)                          # the row outside the grid adds nothing
    # the comparison is not vacuous (figures of the reference, on the CPU)
    tab = mr.table(want)
    inside = lambda v: (v > 0.01) & (v < 0.99)      # noqa: E731
    if (name, n_filt) == ("dsed", 5):
        print(f"case 1: {live.sum()} live, {(tab[live, 3] > 1e-6).sum()} with massSd > 1e-6, {inside(tab[:, 6]).sum()} pBinary inside, {inside(tab[:, 7]).sum()} pPop2 inside")
        assert live.sum() >= 90 and np.all(tab[live, 3] > 1e-6) and inside(tab[:, 6]).sum() >= 90 and inside(tab[:, 7]).sum() >= 100
    if (name, n_filt) == ("parsec", 8):
        print(f"case 2: {inside(tab[:, 6]).sum()} pBinary inside, {inside(tab[:, 1]).sum()} membership inside")
        assert inside(tab[:, 6]).sum() >= 60 and inside(tab[:, 1]).sum() >= 25


# ---- 2. edges of the shapes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_wd", [0, 1, 4, 5])
@pytest.mark.parametrize("n_ms", [1, 64, 65])
def test_star_count_edges(n_ms, n_wd):
    pack_d, cl, pack, _, priors, _ = build_problem("parsec", 4, n_stars=400, wd_frac=0.1, seed=12)
    stage = np.asarray(cl["stage"])
    ms, wd = np.flatnonzero(stage != abi.STAGE_WD)[:n_ms], np.flatnonzero(stage == abi.STAGE_WD)[:n_wd]
    assert len(ms) == n_ms and len(wd) == n_wd
    cl = subset(cl, np.sort(np.concatenate([ms, wd])))
    against_reference(pack_d, cl, pack, abi.make_stars(cl), priors, 1, 2, 2, rows=rows_for(pack_d, cl, 1, 2))


def test_special_stars():
    """A star with every filter unused, one with (all but) no membership prior, one with membership prior 1.  The library
    takes clust_prior in (0, 1] only -- b9_load_stars refuses 0, checked here -- so the star without membership prior carries
    1e-300: its membership is 0 to every tolerance while the star still counts its rows."""
    from base_amd import engine
    pack_d, cl, pack, _, priors, _ = build_problem("parsec", 4, n_stars=70, wd_frac=0.1, seed=12)
    cl = subset(cl, np.arange(70))
    cl["sigma"] = np.array(cl["sigma"], dtype=np.float64)
    cl["clust_prior"] = np.array(cl["clust_prior"], dtype=np.float64)
    ms = np.flatnonzero(np.asarray(cl["stage"]) != abi.STAGE_WD)
    cl["sigma"][ms[3]] = -1.0
    cl["clust_prior"][ms[5]] = 0.0
    cl["clust_prior"][ms[7]] = 1.0
    with pytest.raises(engine.B9Error) as e:
        engine.Engine(pack, abi.make_stars(cl), priors, opts(1, 2, 2))
    assert e.value.code == abi.B9_ERR_INVALID and "clust_prior" in str(e.value)
    cl["clust_prior"][ms[5]] = 1e-300
    got, want = against_reference(pack_d, cl, pack, abi.make_stars(cl), priors, 1, 2, 2)
    assert got[ms[5], 0] == 3 and np.all(got[ms[5], 1:] < 1e-250)        # counted, no membership weight
    assert got[ms[7], 1] == 3.0 and got[ms[3], 0] == 3 and got[ms[3], 2] > 0


@pytest.mark.parametrize("n_eep,K,n_chunks", [(40, 1, 1), (90, 3, 5)])
def test_node_table_edges(n_eep, K, n_chunks):
    """One partial 64-node chunk; five chunks, the last one partial."""
    pack_d, cl, pack, stars, priors, _ = build_problem("parsec", 4, n_stars=70, wd_frac=0.1, seed=12, n_eep=n_eep)
    assert ((int(np.max(pack_d["iso_n_eep"])) - 1) * K + 63) // 64 == n_chunks
    against_reference(pack_d, cl, pack, stars, priors, 1, K, 2)


# ---- 3. tie to b9_sample_mass ----------------------------------------------------------------------------------------------
def test_tie_to_sample_mass():
    from base_amd import engine
    pack_d, cl, pack, stars, priors, _ = build_problem("dsed", 5, n_stars=130, wd_frac=0.1, n_y=3, n_pops=2, seed=12)
    rows = rows_for(pack_d, cl, 2)
    eng = engine.Engine(pack, stars, priors, opts(2, 2, 2))
    try:
        mass, ratio, member, pop = eng.sample_mass(rows, seed=5)
        for r in range(len(rows)):
            acc = eng.star_moments(rows[r:r + 1])
            np.testing.assert_allclose(acc[:, 1], member[r], rtol=1e-12, atol=1e-300)
            assert np.array_equal(acc[:, 0], (mass[r] > 0).astype(float))
    finally:
        eng.close()
    assert np.all(mass[-1] == 0) and (mass[0] > 0).sum() >= 120


# ---- 4. bitwise invariances -------------------------------------------------------------------------------------------------
def test_bitwise_invariances():
    from base_amd import engine
    pack_d, cl, pack, stars, priors, _ = build_problem("dsed", 5, n_stars=130, wd_frac=0.1, n_y=3, n_pops=2, seed=12)
    rows = synth.walker_params(cl["truth"], 40, seed=8, scale=0.3, n_pops=2)
    outside = rows[0].copy(); outside[abi.P_LOGAGE] = pack_d["log_age"][-1] + 1.0
    eng = engine.Engine(pack, stars, priors, opts(2, 2, 2))
    try:
        whole = eng.star_moments(rows)
        assert np.all(whole[:, 0] <= 40) and (whole[:, 0] == 40).sum() >= 120
        # 40 rows in one call = the same rows as 1 + 32 + 7 continued
        acc = eng.star_moments(rows[:1])
        acc = eng.star_moments(rows[1:33], acc)
        acc = eng.star_moments(rows[33:], acc)
        assert np.array_equal(acc, whole)
        # row j alone = the increment it makes inside a batch: a continued call started from zeros returns 0 + x exactly, so
        # row j between rows that contribute nothing (outside the grid) shows its in-batch increment; and a batch's
        # accumulators are the previous ones + that increment, one add
        j = 17
        alone = eng.star_moments(rows[j:j + 1])
        batch = np.tile(outside, (36, 1)); batch[j] = rows[j]              # two chunks; row j at position 17 of the first
        assert np.array_equal(eng.star_moments(batch, np.zeros_like(alone)), alone)
        before, after = eng.star_moments(rows[:j], np.zeros_like(alone)), eng.star_moments(rows[:j + 1], np.zeros_like(alone))
        assert np.array_equal(after, before + alone)
        # repeated calls on one context = a fresh context
        again = eng.star_moments(rows)
        assert np.array_equal(again, whole)
    finally:
        eng.close()
    eng = engine.Engine(pack, stars, priors, opts(2, 2, 2))
    try:
        assert np.array_equal(eng.star_moments(rows), whole)
    finally:
        eng.close()
    # star order: a permuted catalogue gives permuted accumulators
    perm = np.random.default_rng(3).permutation(len(cl["mass1"]))
    cl2 = subset(cl, perm)
    eng = engine.Engine(pack, abi.make_stars(cl2), priors, opts(2, 2, 2))
    try:
        assert np.array_equal(eng.star_moments(rows), whole[perm])
    finally:
        eng.close()


def test_invalid_arguments():
    from base_amd import engine
    pack_d, cl, pack, stars, priors, _ = build_problem("parsec", 4, n_stars=20, seed=12)
    eng = engine.Engine(pack, stars, priors, opts(1, 1, 1))
    try:
        acc = np.zeros((20, abi.MOM_N))
        dp = C.POINTER(C.c_double)
        row = rows_for(pack_d, cl, 1, 1, outside=False)
        assert eng.lib.b9_star_moments(eng._ctx, row.ctypes.data_as(dp), 0, 0, acc.ctypes.data_as(dp)) == abi.B9_ERR_INVALID
        assert eng.lib.b9_star_moments(eng._ctx, None, 1, 0, acc.ctypes.data_as(dp)) == abi.B9_ERR_INVALID
        assert eng.lib.b9_star_moments(eng._ctx, row.ctypes.data_as(dp), 1, 0, None) == abi.B9_ERR_INVALID
    finally:
        eng.close()


# ---- 5. leaves the sampler alone --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [abi.MODE_GIVEN_MASS, abi.MODE_MARGINALISED])
def test_sampler_blocks_are_untouched(mode):
    from base_amd import engine, mcmc
    pack_d, cl, pack, stars, priors, _ = build_problem("parsec", 8, n_stars=130, wd_frac=0.1, seed=12)
    options = opts(1, 2, 2, mode)
    free = np.array(mcmc.DEFAULT_FREE)
    chol = np.diag([mcmc.DEFAULT_STEP[k] for k in free]) * 0.3
    start = synth.walker_params(cl["truth"], 4, seed=2, scale=0.3)
    rows = rows_for(pack_d, cl, 1)

    def run(interleave):
        eng = engine.Engine(pack, stars, priors, options)
        try:
            lp0 = eng.logpost(start)
            h = eng.mcmc_submit(start, lp0, np.arange(4), free, chol, 11, 0, 6, asynchronous=True)
            if interleave:
                with pytest.raises(Exception) as e:                        # B9_ERR_STATE: a block is outstanding
                    eng.star_moments(rows)
                assert e.value.code == abi.B9_ERR_STATE and "outstanding" in str(e.value)
            first = [np.array(x) for x in eng.mcmc_collect(h)[:4]]
            if interleave:
                acc = eng.star_moments(rows)
                assert (acc[:, 0] == 3).sum() >= 100
            h = eng.mcmc_submit(start, lp0, np.arange(4), free, chol, 11, 6, 6, cont=True, asynchronous=True)
            second = [np.array(x) for x in eng.mcmc_collect(h)[:4]]
        finally:
            eng.close()
        return first + second

    for a, b in zip(run(False), run(True)):
        assert np.array_equal(a, b)


# ---- 6. statistics against the device's own draws ---------------------------------------------------------------------------
def test_statistics_against_device_draws():
    """Case 1, one parameter row repeated R = 1000 times: b9_sample_mass gives 1000 independent draws per star.  The counts
    of ratio > 0 and of pop == 1 against Binomial(R, pBinary) / Binomial(R, pPop2) (two-sided exact, p >= 1e-7 each), and
    the mean drawn mass against the table's mass with the reference's variance, |z| <= 6, for the stars whose reference
    skewness keeps |gamma_1| / sqrt(R) <= 0.3.  The same checks run on numpy draws from the reference weights, and reject
    mutated references, in tests/test_moments_host.py (there: 243 tests, smallest p 0.018; 92 guarded stars, largest |z| 2.0;
    on the device's draws, measured once: smallest p 6.1e-4, largest |z| 3.2)."""
    from base_amd import engine
    R = 1000
    pack_d, cl, pack, stars, priors, _ = build_problem("dsed", 5, n_stars=130, wd_frac=0.1, n_y=3, n_pops=2, seed=12)
    row = rows_for(pack_d, cl, 2, outside=False)[:1]
    eng = engine.Engine(pack, stars, priors, opts(2, 2, 2))
    try:
        acc = eng.star_moments(row)
        mass, ratio, member, pop = eng.sample_mass(np.repeat(row, R, axis=0), seed=20240611)
        tab = engine.star_table(acc)
    finally:
        eng.close()
    nodes = mr.star_nodes(pack_d, cl, row[0], 2, 2, 2)
    ref_mo = [mr.skewness(nd) if len(nd[0]) else None for nd in nodes]
    p = mr.binomial_pvalues(tab, acc, (ratio > 0).sum(axis=0), (pop == 1).sum(axis=0), R, 2)
    z = mr.mass_z(tab, mass.mean(axis=0), ref_mo, R)
    print(f"{len(p)} binomial tests, smallest p {p.min():.3g}; {len(z)} guarded stars, largest |z| {np.abs(z).max():.3g}")
    assert len(p) >= 150 and p.min() >= mr.P_MIN
    assert len(z) >= 60 and np.abs(z).max() <= mr.Z_MAX


# ---- 7. every instance ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pops", [1, 2])
@pytest.mark.parametrize("n_filt", [1, 3, 4, 5, 8, 9, 16])
def test_every_instance(n_filt, n_pops):
    pack_d, cl, pack, stars, priors, _ = build_problem("dsed", n_filt, n_stars=70, wd_frac=0.1, n_y=3 if n_pops == 2 else 1, n_pops=n_pops, seed=12)
    against_reference(pack_d, cl, pack, stars, priors, n_pops, 2, 2, rows=rows_for(pack_d, cl, n_pops, 2, outside=False))


# ---- 8. the CLI ---------------------------------------------------------------------------------------------------------------
def test_cli_star_summary(tmp_path):
    """simCluster (200 stars) -> scatterCluster -> singlePopMcmc (short) -> starSummary: the file parses, equals
    engine.star_table(Engine.star_moments(stage-3 rows)) to the printed precision, and the member stars' mass lies within
    3 massSd + one grid step of the true primary mass for at least 90 % of the stars with membership > 0.9."""
    from base_amd import build, engine, host_build, hostlib
    build.build_hip()
    host_build.build_host()
    K = Q = 4                                            # the program's defaults
    pack_d = synth.make_pack("parsec", 8, n_feh=4, n_age=8, n_eep=90)
    truth = synth.default_params(pack_d)
    truth[abi.P_IFMR_INTERCEPT], truth[abi.P_IFMR_SLOPE], truth[abi.P_IFMR_QUAD] = 0.77, 0.08, 0.0   # the session's defaults
    root = synth.write_models_dir(pack_d, str(tmp_path / "models"))
    base = str(tmp_path / "run")
    y_true = synth.write_yaml(str(tmp_path / "truth.yaml"), base + ".sim.scatter", root, base, truth, seed=17)
    r = _cli("simCluster", "--config", y_true, "--nStars", "200", "--percentBinary", "30", "--minMass", "0.4")
    assert r.returncode == 0, r.stderr
    r = _cli("scatterCluster", "--config", y_true, "--sigmaFloor", "0.01", "--sigmaAtLimit", "0.05", "--faintLimit", "45")
    assert r.returncode == 0, r.stderr
    start = truth.copy()
    start[abi.P_LOGAGE] += 0.004; start[abi.P_MOD] += 0.01; start[abi.P_FEH] -= 0.01
    fit = str(tmp_path / "fit")
    y = synth.write_yaml(str(tmp_path / "fit.yaml"), base + ".sim.scatter", root, fit, start, burn=1000, run=100, walkers=4)
    r = _cli("singlePopMcmc", "--config", y, "--priorFe_H", repr(float(truth[abi.P_FEH])), "--priorDistMod", repr(float(truth[abi.P_MOD])),
             "--priorAv", repr(float(truth[abi.P_ABS])))
    assert r.returncode == 0, r.stderr
    r = _cli("starSummary", "--config", y)
    assert r.returncode == 0, r.stderr
    assert "star rows/s" in r.stderr

    cl = _read_phot(base + ".sim.scatter")
    phot_ids = [ln.split()[0] for ln in open(base + ".sim.scatter").read().splitlines()[1:]]
    ids, cols, tab = hostlib.read_star_summary(fit + ".starSummary")
    assert ids == phot_ids and cols == ["rows", "member", "mass", "massSd", "massRatio", "massRatioSd", "pBinary"]
    rows = hostlib.read_res_rows(fit + ".res", start, 3)
    assert len(rows) == 100 * 4
    eng = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cl), synth.default_priors(pack_d, truth), opts(1, K, Q))
    try:
        want = engine.star_table(eng.star_moments(rows))
        _, iso_mass, _, tip = eng.derive_isochrone(truth)
    finally:
        eng.close()
    np.testing.assert_allclose(tab, want[:, :7], rtol=0, atol=6e-7)        # %.6f
    assert np.all(tab[:, 0] == len(rows))

    # recovery against the truth in .sim.out
    sim = open(base + ".sim.out").read().splitlines()
    col = {n: i for i, n in enumerate(sim[0].split())}
    true_mass = {ln.split()[0]: float(ln.split()[col["mass1"]]) for ln in sim[1:]}
    m_true = np.array([true_mass[i] for i in ids])

    def grid_step(m):                                                    # the node spacing at mass m
        if m > tip:
            return (pack_d["m_wd_up"] - tip) / (8 * K)
        e = int(np.clip(np.searchsorted(iso_mass, m) - 1, 0, len(iso_mass) - 2))
        return (iso_mass[e + 1] - iso_mass[e]) / K
    step = np.array([grid_step(m) for m in m_true])
    sel = tab[:, 1] > 0.9
    ok = np.abs(tab[sel, 2] - m_true[sel]) <= 3 * tab[sel, 3] + step[sel]
    print(f"recovery: {ok.mean():.1%} of {sel.sum()} stars with membership > 0.9 have their true primary mass within 3 massSd + one grid step")
    assert sel.sum() >= 100 and ok.mean() >= 0.9
