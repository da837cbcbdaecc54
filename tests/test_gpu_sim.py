"""b9_predict_mags and the simulation loop on the GPU: predictions equal the numpy forward model (synth.forward_mags),
fed back as observations they give the oracle's chi^2 = 0 likelihood, bits do not depend on batching, the call leaves a
sampler chain alone; simCluster writes what its restated draws and the forward model give, and simCluster ->
scatterCluster -> singlePopMcmc / multiPopMcmc recovers the truth."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
from base_amd import abi, engine, host_build, hostlib, mcmc, synth
from sim_check import branch_systems as _systems, forward_by_pop as _want, isochrone_tips as _tips

pytestmark = pytest.mark.gpu

NOFLUX = abi.MAG_NOFLUX


@pytest.fixture(scope="module", autouse=True)
def built():
    from base_amd import build
    build.build_hip()
    host_build.build_host()


def _cli(name, *args):
    return subprocess.run([os.path.join(host_build.BIN, name), *args], capture_output=True, text=True, timeout=900)


@pytest.mark.parametrize("name,nf,n_y,ragged", [("parsec", 8, 1, False), ("dsed", 5, 3, True)])
def test_predict_matches_forward_model(name, nf, n_y, ragged):
    pack_d = synth.make_pack(name, nf, n_y=n_y, n_feh=4, n_age=8, n_eep=90, wd_ragged=ragged)
    row = synth.default_params(pack_d)
    pack = abi.make_pack(pack_d)
    n_pops = 2 if n_y > 1 else 1
    isos = _tips(pack, row, n_pops)
    m1, q, wt, pop = _systems(isos, pack_d["m_wd_up"], n_pops, np.random.default_rng(3))
    eng = engine.Engine(pack)
    mags, stage = eng.predict_mags(row, m1, q, wt, pop if n_pops == 2 else None)
    want = _want(pack_d, row, m1, q, wt, pop)
    first = np.array([isos[k][1][0] for k in pop])
    tip = np.array([isos[k][3] for k in pop])
    dark1 = (m1 < first) | (m1 > pack_d["m_wd_up"])
    dark = dark1 & ((q == 0) | (q * m1 < first))
    assert dark.sum() >= 3 * n_pops and (~dark).sum() >= 80 * n_pops
    assert np.all(mags[dark] == NOFLUX)                                  # exact
    np.testing.assert_allclose(mags[~dark], want[~dark], rtol=0, atol=1e-10)
    want_stage = np.where(m1 <= tip, abi.STAGE_MSRG, np.where(m1 <= pack_d["m_wd_up"], abi.STAGE_WD, abi.STAGE_NSBH))
    np.testing.assert_array_equal(stage, want_stage)
    eng.close()


def test_predictions_fed_back_give_the_oracle_zero_chi2_likelihood():
    pack_d = synth.make_pack("parsec", 8, n_feh=4, n_age=8, n_eep=90)
    row = synth.default_params(pack_d)
    pack = abi.make_pack(pack_d)
    tip = _tips(pack, row, 1)[0][3]
    m1, q, wt, _ = hostlib.sim_draw_systems(5, 0, 800, [tip], percent_binary=30.0, percent_db=20.0)
    eng = engine.Engine(pack)
    mags, stage = eng.predict_mags(row, m1, q, wt)
    ok = np.all(np.isfinite(mags) & (mags != NOFLUX), axis=1)
    assert ok.sum() > 500 and np.any(stage[ok] == abi.STAGE_WD)
    n, sig, p = int(ok.sum()), 1e-4, 0.9
    lo, hi = mags[ok].min(axis=0) - 0.5, mags[ok].max(axis=0) + 0.5
    cl = dict(n_filt=8, obs=mags[ok], sigma=np.full((n, 8), sig), mass1=m1[ok], mass_ratio=q[ok], clust_prior=np.full(n, p),
              stage=stage[ok], wd_type=wt[ok], filter_prior_min=lo, filter_prior_max=hi)
    stars = abi.make_stars(cl)
    _, ps = oracle.Oracle(pack, stars, synth.default_priors(pack_d, row), abi.make_options()).logpost(row[None, :], perstar=True)
    lib = oracle.load()
    lib.b9o_log_mass_norm.restype = C.c_double
    lib.b9o_log_mass_norm.argtypes = [C.c_double]
    lib.b9o_log_prior_mass.restype = C.c_double
    lib.b9o_log_prior_mass.argtypes = [C.c_double, C.c_double]
    lmn = lib.b9o_log_mass_norm(pack_d["m_wd_up"])
    # given-mass mode: a member's likelihood also carries the mass prior at its catalogue mass
    lpm = np.array([lib.b9o_log_prior_mass(lmn, m) for m in m1[ok]])
    la = np.log(1 - p) - np.sum(np.log(hi - lo))
    lb = np.log(p) + lpm + 8 * (-0.5 * np.log(2 * np.pi * sig * sig))
    np.testing.assert_allclose(ps[0], np.logaddexp(la, lb), rtol=1e-12, atol=0)
    eng.close()


def test_predict_bits_batching_states_and_chain():
    from conftest import build_problem
    pack_d, cl, pack, stars, priors, options = build_problem("parsec", 8, 400, wd_frac=0.05)
    row = synth.default_params(pack_d)
    tip = _tips(pack, row, 1)[0][3]
    m1, q, wt, _ = hostlib.sim_draw_systems(8, 0, 3000, [tip], percent_binary=40.0, percent_db=30.0)
    m1[::97] = np.random.default_rng(1).uniform(tip, 8.0, m1[::97].size)     # WD primaries in the same waves as MS ones
    eng = engine.Engine(pack, stars, priors, options)
    whole, st_whole = eng.predict_mags(row, m1, q, wt)
    parts = [eng.predict_mags(row, m1[a:b], q[a:b], wt[a:b]) for a, b in ((0, 1), (1, 1777), (1777, 3000))]
    assert np.array_equal(np.concatenate([x[0] for x in parts]), whole) and np.array_equal(np.concatenate([x[1] for x in parts]), st_whole)
    perm = np.random.default_rng(2).permutation(3000)
    pm, ps_ = eng.predict_mags(row, m1[perm], q[perm], wt[perm])
    assert np.array_equal(pm, whole[perm]) and np.array_equal(ps_, st_whole[perm])
    assert np.any(st_whole == abi.STAGE_WD)
    # a row outside the grid: NOFLUX / DNE, not an error
    off = row.copy()
    off[abi.P_LOGAGE] = 20.0
    om, os_ = eng.predict_mags(off, m1[:50], q[:50], wt[:50])
    assert np.all(om == NOFLUX) and np.all(os_ == abi.STAGE_DNE)
    # no pack: B9_ERR_STATE
    bare = engine.Engine()
    with pytest.raises(engine.B9Error) as ei:
        bare.predict_mags(row, m1[:4], q[:4])
    assert ei.value.code == abi.B9_ERR_STATE
    bare.close()
    # the chain: block A, then a CONTINUE block B -- with and without a predict call between them -- the same bits; and a
    # predict call while a block is outstanding is B9_ERR_STATE
    free = np.array(mcmc.DEFAULT_FREE)
    chol = np.diag([mcmc.DEFAULT_STEP[k] for k in free]) * 0.5
    start = synth.walker_params(row, 4)

    def chain(with_predict):
        e = engine.Engine(pack, stars, priors, options)
        lp0 = e.logpost(start)
        e.mcmc_collect(e.mcmc_submit(start, lp0, np.arange(4), free, chol, 9, 0, 8, record=True, asynchronous=True))
        if with_predict:
            assert np.array_equal(e.predict_mags(row, m1, q, wt)[0], whole)
        hb = e.mcmc_submit(start, lp0, np.arange(4), free, chol, 9, 8, 8, record=True, cont=True, asynchronous=True)
        if with_predict:
            with pytest.raises(engine.B9Error) as ei:
                e.predict_mags(row, m1[:4], q[:4])
            assert ei.value.code == abi.B9_ERR_STATE
        out = e.mcmc_collect(hb)
        e.close()
        return out
    a, b = chain(False), chain(True)
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x, y)
    assert a[4] == b[4]
    eng.close()


def _truth_row(pack_d):
    row = synth.default_params(pack_d)
    row[abi.P_IFMR_INTERCEPT], row[abi.P_IFMR_SLOPE], row[abi.P_IFMR_QUAD] = 0.77, 0.08, 0.0   # open_session's defaults
    return row


def test_simcluster_cli_matches_restated_draws_and_forward_model(tmp_path):
    pack_d = synth.make_pack("parsec", 8, n_feh=4, n_age=8, n_eep=90)
    row = _truth_row(pack_d)
    root = synth.write_models_dir(pack_d, str(tmp_path / "models"))
    y = synth.write_yaml(str(tmp_path / "b.yaml"), "unused.phot", root, str(tmp_path / "run"), row, seed=31)
    args = ["--config", y, "--nStars", "400", "--nFieldStars", "25", "--percentBinary", "30", "--percentDB", "20", "--minMassRatio", "0.1"]
    r = _cli("simCluster", *args)
    assert r.returncode == 0, r.stderr
    path = str(tmp_path / "run.sim.out")
    head = open(path).readline().split()
    assert head == ["id"] + pack_d["filters"] + ["mass1", "massRatio", "stage", "wdType", "pop", "member"]
    t = np.loadtxt(path, skiprows=1)
    tip = _tips(abi.make_pack(pack_d), row, 1)[0][3]
    m1, q, wt, pop = hostlib.sim_draw_systems(31, 0, 425, [tip], percent_binary=30.0, percent_db=20.0, min_mass_ratio=0.1)
    np.testing.assert_array_equal(t[:, 0], np.arange(425))
    np.testing.assert_allclose(t[:, 9], m1, rtol=0, atol=1e-11)
    np.testing.assert_allclose(t[:, 10], q, rtol=0, atol=1e-11)
    np.testing.assert_array_equal(t[:, 12:14], np.stack([wt, pop], axis=1))
    np.testing.assert_array_equal(t[:, 14], (np.arange(425) < 400).astype(float))
    np.testing.assert_array_equal(t[:, 11], np.where(m1 <= tip, 1, np.where(m1 <= 8.0, 3, 4)))
    want = synth.forward_mags(pack_d, row, m1[:400], q[:400], wt[:400])
    mem = t[:400, 1:9]
    dark = mem == NOFLUX
    assert np.all(dark == dark[:, :1]) and np.all(m1[:400][dark[:, 0]] < 0.2)
    np.testing.assert_allclose(mem[~dark], want[~dark], rtol=0, atol=1e-9)
    live = want[~dark[:, 0]]
    f = hostlib.sim_field_mags(31, 400, 25, live.min(axis=0) - 0.5, live.max(axis=0) + 0.5)
    np.testing.assert_allclose(t[400:, 1:9], f, rtol=0, atol=1e-9)
    first = open(path, "rb").read()
    assert _cli("simCluster", *args).returncode == 0
    assert open(path, "rb").read() == first                  # a rerun is byte-identical
    r = _cli("simCluster", *args, "--logAge", "20.0")
    assert r.returncode != 0 and "outside the model grid" in r.stderr


def _read_phot(path):
    lib = hostlib.load()
    h, view = C.c_void_p(), abi.b9_stars()
    buf = C.create_string_buffer(512)
    assert lib.b9h_read_phot(path.encode(), -1e300, 1e300, 0, C.byref(h), C.byref(view), buf, 512) == 0, lib.b9h_last_error()
    n, nf = view.n_stars, view.n_filt
    g = lambda p, k: np.ctypeslib.as_array(p, shape=(k,)).copy()     # noqa: E731
    d = dict(n_filt=nf, obs=g(view.obs, n * nf), sigma=g(view.sigma, n * nf), mass1=g(view.mass1, n), mass_ratio=g(view.mass_ratio, n),
             clust_prior=g(view.clust_prior, n), stage=g(view.stage, n), wd_type=g(view.wd_type, n),
             filter_prior_min=g(view.filter_prior_min, nf), filter_prior_max=g(view.filter_prior_max, nf))
    lib.b9h_free_phot(h)
    return d


@pytest.mark.parametrize("prog,n_y,mode", [("singlePopMcmc", 1, "givenMass"), ("singlePopMcmc", 1, "marginalised"),
                                           ("multiPopMcmc", 3, "givenMass")])
def test_simulate_scatter_fit_recovers_truth(tmp_path, prog, n_y, mode):
    """simCluster -> scatterCluster -> singlePopMcmc / multiPopMcmc, judged as test_mcmc_cli_runs_and_recovers_truth is."""
    n_pops = 2 if prog == "multiPopMcmc" else 1
    pack_d = synth.make_pack("dsed", 8, n_y=n_y, n_feh=4, n_age=8, n_eep=90)
    truth = _truth_row(pack_d)
    root = synth.write_models_dir(pack_d, str(tmp_path / "models"))
    base = str(tmp_path / "run")
    y_true = synth.write_yaml(str(tmp_path / "truth.yaml"), base + ".sim.scatter", root, base, truth, ms_model="dsed", seed=17)
    pops = ["--nPops", "2", "--startingYA", repr(float(truth[abi.P_Y])), "--startingYB", repr(float(truth[abi.P_Y2])),
            "--startingLambda", "0.5"] if n_pops == 2 else []
    r = _cli("simCluster", "--config", y_true, "--nStars", "2000", "--nFieldStars", "40", "--percentBinary", "30", "--percentDB", "10",
             "--minMass", "0.25", *pops)
    assert r.returncode == 0, r.stderr
    # (two populations: wider errors -- seven free parameters along the synthetic grids' near-degenerate ridges mix slowly
    # under 0.01 mag, as test_mcmc_cli_runs_and_recovers_truth's clusters have 0.01 - 0.05)
    floor = "0.03" if n_pops == 2 else "0.01"
    r = _cli("scatterCluster", "--config", y_true, "--sigmaFloor", floor, "--sigmaAtLimit", "0.05", "--faintLimit", "26")
    assert r.returncode == 0, r.stderr
    # start AWAY from the truth (further in the marginalised mode: integrating over the masses flattens the posterior)
    far = 1.5 if mode == "marginalised" else 1.0
    start = truth.copy()
    start[abi.P_LOGAGE] += 0.008 * far; start[abi.P_MOD] += 0.015 * far; start[abi.P_FEH] -= 0.02 * far
    y = synth.write_yaml(str(tmp_path / "fit.yaml"), base + ".sim.scatter", root, str(tmp_path / "fit"), start, ms_model="dsed",
                         burn=6000 if n_pops == 2 else 4000, run=1500, walkers=4)
    extra = ["--priorFe_H", repr(float(truth[abi.P_FEH])), "--priorDistMod", repr(float(truth[abi.P_MOD])),
             "--priorAv", repr(float(truth[abi.P_ABS]))]
    margs = ["--mode", "marginalised", "--margIsoIncrem", "4", "--nMassRatios", "4"] if mode == "marginalised" else []
    if n_pops == 2:
        extra += ["--startingYA", repr(float(truth[abi.P_Y])), "--startingYB", repr(float(truth[abi.P_Y2])), "--startingLambda", "0.5"]
    r = _cli(prog, "--config", y, *extra, *margs)
    assert r.returncode == 0, r.stderr
    res_path = str(tmp_path / "fit.res")
    head = open(res_path).readline().split()
    res = np.loadtxt(res_path, skiprows=1)
    main = res[res[:, -1] == 3]
    assert len(main) == 1500 * 4 and np.all(np.isfinite(main[:, -2]))
    col = {n: i for i, n in enumerate(head)}
    cl = _read_phot(base + ".sim.scatter")
    assert cl["mass1"].size > 1800
    pri = synth.default_priors(pack_d, truth, n_pops)
    for k in (abi.P_Y, abi.P_Y2):
        pri.var[k] = 0.0
    opts = abi.make_options(abi.MODE_MARGINALISED if mode == "marginalised" else abi.MODE_GIVEN_MASS, n_pops, 4, 4)
    orc = oracle.Oracle(abi.make_pack(pack_d), abi.make_stars(cl), pri, opts)
    row = truth.copy()
    for name, i in col.items():
        key = {"logAge": abi.P_LOGAGE, "FeH": abi.P_FEH, "modulus": abi.P_MOD, "absorption": abi.P_ABS, "Y": abi.P_Y,
               "YA": abi.P_Y, "YB": abi.P_Y2, "lambda": abi.P_LAMBDA}.get(name)
        if key is not None:
            row[key] = main[-1, i]
    want = orc.logpost(row[None, :])[0]
    assert abs(main[-1, -2] - want) <= 2e-4 * max(1.0, abs(want))      # .res holds 6 decimals of each parameter
    t_row, s_row = row.copy(), row.copy()
    for k in (abi.P_LOGAGE, abi.P_FEH, abi.P_MOD, abi.P_ABS, abi.P_Y, abi.P_Y2, abi.P_LAMBDA):
        t_row[k] = truth[k]; s_row[k] = truth[k]
    for k in (abi.P_LOGAGE, abi.P_FEH, abi.P_MOD):
        s_row[k] = start[k]
    lp_truth, lp_start = orc.logpost(np.stack([t_row, s_row]))
    assert lp_start < lp_truth - (20.0 if mode == "marginalised" else 50.0), (lp_start, lp_truth)
    assert main[:, -2].mean() > lp_truth - (6.0 + 0.5 * (len(head) - 2)), (main[:, -2].mean(), lp_truth)
    assert abs(main[:, col["logAge"]].mean() - truth[abi.P_LOGAGE]) < abs(start[abi.P_LOGAGE] - truth[abi.P_LOGAGE])
