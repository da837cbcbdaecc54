"""simCluster / scatterCluster host side, CPU only: the counter-based draws of libbase9host equal a numpy restatement built
on base_amd.mcmc's Philox4x32-10, follow their distributions, and scatterCluster turns a hand-written .sim.out into the
.phot rows docs/FORMATS.md states (noise, cuts at their boundaries) without a GPU; the settings resolve and are checked."""
import math
import os
import subprocess

import numpy as np
import pytest

from base_amd import abi, host_build, hostlib, mcmc, synth

BIN = os.path.join(host_build.BIN)
MU, SIG = -1.02, 0.677


@pytest.fixture(scope="module", autouse=True)
def built():
    from base_amd import build
    build.build_hip()
    host_build.build_host()


def _philox(seed, i, purpose, j):
    i = np.asarray(i, dtype=np.uint64)
    return mcmc.philox4x32((i & np.uint64(0xFFFFFFFF)).astype(np.uint32), (i >> np.uint64(32)).astype(np.uint32),
                           np.uint32(purpose), np.uint32(j), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def _phi(x):
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


def restate_systems(seed, i0, n, tip, min_mass, max_mass, pb, mmr, pdb, n_pops, lam):
    """docs/FORMATS.md "Simulation draws", purposes 0-3, in numpy."""
    ids = np.arange(i0, i0 + n, dtype=np.uint64)
    zlow, zup = (math.log10(min_mass) - MU) / SIG, (math.log10(max_mass) - MU) / SIG
    m1 = np.full(n, np.nan)
    for j in range(4096):
        todo = np.isnan(m1)
        if not todo.any():
            break
        r = _philox(seed, ids, 0, j)
        z = np.sqrt(-2.0 * np.log(mcmc._u01(r[0], r[1]))) * np.cos(2.0 * np.pi * mcmc._u01(r[2], r[3]))
        ok = todo & (z >= zlow) & (z <= zup)
        m1[ok] = 10.0 ** (MU + SIG * z[ok])
    r = _philox(seed, ids, 3, 0)
    pop = ((mcmc._u01(r[0], r[1]) >= lam) if n_pops == 2 else np.zeros(n, bool)).astype(np.int32)
    r = _philox(seed, ids, 1, 0)
    q = np.where(mcmc._u01(r[0], r[1]) < pb / 100.0, mmr + (1.0 - mmr) * mcmc._u01(r[2], r[3]), 0.0)
    tips = np.array([tip[0], tip[-1]])
    q[m1 > tips[pop]] = 0.0
    r = _philox(seed, ids, 2, 0)
    wt = (mcmc._u01(r[0], r[1]) < pdb / 100.0).astype(np.int32)
    return m1, q, wt, pop


def restate_uniform_pairs(seed, ids, purpose, nf):
    """u[n, nf]: filters 2k, 2k+1 from draw j = k of `purpose`"""
    ids = np.asarray(ids, dtype=np.uint64)
    u = np.empty((ids.size, nf))
    for k in range((nf + 1) // 2):
        r = _philox(seed, ids, purpose, k)
        u[:, 2 * k] = mcmc._u01(r[0], r[1])
        if 2 * k + 1 < nf:
            u[:, 2 * k + 1] = mcmc._u01(r[2], r[3])
    return u


def restate_noise(seed, ids, mags, floor, at_limit, faint):
    ids = np.asarray(ids, dtype=np.uint64)
    n, nf = mags.shape
    z = np.empty((n, nf))
    for k in range((nf + 1) // 2):
        r = _philox(seed, ids, 5, k)
        rad, ang = np.sqrt(-2.0 * np.log(mcmc._u01(r[0], r[1]))), 2.0 * np.pi * mcmc._u01(r[2], r[3])
        z[:, 2 * k] = rad * np.cos(ang)
        if 2 * k + 1 < nf:
            z[:, 2 * k + 1] = rad * np.sin(ang)
    t = at_limit * 10.0 ** (0.2 * (mags - faint))
    sigma = np.sqrt(floor ** 2 + t ** 2)
    return sigma, mags + sigma * z


@pytest.mark.parametrize("n_pops", [1, 2])
def test_draws_equal_the_numpy_restatement(n_pops):
    seed = (7 << 32) | 12345
    args = dict(min_mass=0.15, max_mass=7.5, percent_binary=40.0, min_mass_ratio=0.2, percent_db=25.0, n_pops=n_pops, lam=0.6)
    tip = [1.7, 1.9] if n_pops == 2 else [1.7]
    got = hostlib.sim_draw_systems(seed, 1000, 3000, tip, **args)
    want = restate_systems(seed, 1000, 3000, tip, 0.15, 7.5, 40.0, 0.2, 25.0, n_pops, 0.6)
    np.testing.assert_allclose(got[0], want[0], rtol=1e-13, atol=0)
    np.testing.assert_allclose(got[1], want[1], rtol=1e-13, atol=0)
    np.testing.assert_array_equal(got[2], want[2])
    np.testing.assert_array_equal(got[3], want[3])
    # a system's values depend on (seed, i, settings) only: a sub-range drawn alone is the same bits
    part = hostlib.sim_draw_systems(seed, 2000, 17, tip, **args)
    for a, b in zip(part, got):
        np.testing.assert_array_equal(a, b[1000:1017])
    lo, hi = np.array([10.0, 11.0, 12.0]), np.array([15.0, 18.0, 12.5])
    f = hostlib.sim_field_mags(seed, 50, 400, lo, hi)
    np.testing.assert_allclose(f, lo + (hi - lo) * restate_uniform_pairs(seed, np.arange(50, 450), 4, 3), rtol=1e-13, atol=0)
    assert np.all((f >= lo) & (f <= hi))


def test_draws_follow_their_distributions():
    n, seed, tip, mmr = 40000, 99, 1.3, 0.25
    m1, q, wt, pop = hostlib.sim_draw_systems(seed, 0, n, [tip, 1.5], min_mass=0.2, max_mass=6.0, percent_binary=30.0,
                                              min_mass_ratio=mmr, percent_db=15.0, n_pops=2, lam=0.7)
    # m1: Kolmogorov-Smirnov against the truncated log-normal in log10 m
    zl, zu = (math.log10(0.2) - MU) / SIG, (math.log10(6.0) - MU) / SIG
    z = np.sort((np.log10(m1) - MU) / SIG)
    cdf = (np.array([_phi(v) for v in z]) - _phi(zl)) / (_phi(zu) - _phi(zl))
    ecdf_hi, ecdf_lo = np.arange(1, n + 1) / n, np.arange(n) / n
    d = max(np.max(ecdf_hi - cdf), np.max(cdf - ecdf_lo))
    assert d < 1.63 / math.sqrt(n), d                   # 1 % critical value
    assert m1.min() >= 0.2 * (1 - 1e-12) and m1.max() <= 6.0 * (1 + 1e-12)

    def within_4_sigma(k, m, p):
        assert abs(k - m * p) <= 4.0 * math.sqrt(m * p * (1 - p)), (k, m, p)
    below = m1 <= np.where(pop == 1, 1.5, tip)
    within_4_sigma(int(np.sum(q[below] > 0)), int(below.sum()), 0.30)
    within_4_sigma(int(wt.sum()), n, 0.15)
    within_4_sigma(int(pop.sum()), n, 0.30)
    # q uniform on [minMassRatio, 1] for the binaries, 0 above the population's tip
    qb = np.sort(q[q > 0])
    assert qb.min() >= mmr and qb.max() <= 1.0
    u = (qb - mmr) / (1 - mmr)
    d = np.max(np.abs(u - (np.arange(1, u.size + 1) - 0.5) / u.size))
    assert d < 1.63 / math.sqrt(u.size) + 0.5 / u.size, d
    assert np.all(q[~below] == 0.0) and (~below).sum() > 100


def test_draws_reject_a_bad_support():
    with pytest.raises(hostlib.HostError, match="less than 1e-3"):
        hostlib.sim_draw_systems(1, 0, 10, [1.0], min_mass=7.9, max_mass=8.0)
    with pytest.raises(hostlib.HostError, match="percentBinary"):
        hostlib.sim_draw_systems(1, 0, 10, [1.0], percent_binary=101.0)


def _sim_out(path, filters, rows):
    with open(path, "w") as f:
        f.write("id " + " ".join(filters) + " mass1 massRatio stage wdType pop member\n")
        for r in rows:
            f.write(" ".join(str(v) for v in r) + "\n")


def _run(prog, *args, env=None):
    return subprocess.run([os.path.join(BIN, prog), *args], capture_output=True, text=True, timeout=120, env=env)


def test_scatter_cluster_noise_cuts_and_phot(tmp_path):
    """A hand-written .sim.out through scatterCluster with no GPU visible: noise = the restatement, every cut at its boundary."""
    filters = ["B", "V", "I"]
    nf_ = abi.MAG_NOFLUX
    # id  B V I  mass1 q stage wdType pop member;  relevantFilt = 1 (V), limits [12, 20], limitS2N 20
    rows = [
        (0, 13.0, 12.0, 11.5, 1.0, 0.0, 1, 0, 0, 1),          # V at the bright limit: kept
        (1, 21.0, 20.0, 19.0, 0.8, 0.5, 1, 0, 0, 1),          # V at the faint limit: kept if S/N allows (it does)
        (2, 12.5, 11.9999, 11.0, 1.2, 0.0, 1, 0, 0, 1),       # brighter than the bright limit: dropped
        (3, 21.5, 20.0001, 19.5, 0.7, 0.0, 1, 0, 0, 1),       # fainter than the faint limit: dropped
        (4, nf_, 15.0, 14.0, 0.09, 0.0, 1, 0, 0, 1),          # one NOFLUX filter: dropped
        (5, 16.0, 15.0, 14.0, 9.0, 0.0, 4, 0, 0, 1),          # NS/BH: dropped
        (6, 16.0, 15.0, 14.0, 1.0, 0.0, 9, 0, 0, 1),          # DNE: dropped
        (7, 17.0, 16.0, 15.0, 2.5, 0.0, 3, 1, 1, 1),          # WD, DB: kept
        (40, 18.0, 17.0, 16.0, 0.5, 0.3, 1, 0, 0, 0),         # a field star: kept, member column does not matter
    ]
    base = str(tmp_path / "run")
    _sim_out(base + ".sim.out", filters, rows)
    floor, at_limit, faint, seed = 0.01, 0.05, 20.0, 555
    # S/N at V = 20: 1.0857 / sqrt(0.01^2 + 0.05^2) = 21.29; at 20.0001 it would barely differ -- the limit is set just below
    s2n_limit = 1.0857 / math.sqrt(floor ** 2 + at_limit ** 2) - 1e-9
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = _run("scatterCluster", "--outputFileBase", base, "--brightLimit", "12", "--faintLimit", "20", "--relevantFilt", "1",
             "--limitS2N", repr(s2n_limit), "--sigmaFloor", repr(floor), "--sigmaAtLimit", repr(at_limit), "--scatterSeed", str(seed),
             "--memberPrior", "0.85", env=env)
    assert r.returncode == 0, r.stderr
    assert "4 of 9 systems kept" in r.stderr
    txt = open(base + ".sim.scatter").read().splitlines()
    assert txt[0].split() == ["id", "B", "V", "I", "sigB", "sigV", "sigI", "mass1", "massRatio", "stage", "CMprior", "useDBI", "wdType"]
    got = np.array([[float(v) for v in ln.split()] for ln in txt[1:]])
    kept = [0, 1, 7, 40]
    np.testing.assert_array_equal(got[:, 0], kept)
    src = {r_[0]: r_ for r_ in rows}
    mags = np.array([src[i][1:4] for i in kept], dtype=np.float64)
    sigma, obs = restate_noise(seed, kept, mags, floor, at_limit, faint)
    np.testing.assert_allclose(got[:, 1:4], obs, rtol=0, atol=1e-9)
    np.testing.assert_allclose(got[:, 4:7], sigma, rtol=0, atol=1e-9)
    # the library's own noise is the restatement to rounding
    s2, o2 = hostlib.scatter(seed, kept, mags, floor, at_limit, faint)
    np.testing.assert_allclose(s2, sigma, rtol=1e-13)
    np.testing.assert_allclose(o2, obs, rtol=1e-13)
    np.testing.assert_array_equal(got[:, 9], [1, 1, 3, 1])
    assert np.all(got[:, 10] == 0.85) and np.all(got[:, 11] == 1)
    np.testing.assert_array_equal(got[:, 12], [0, 0, 1, 0])
    # a limit S/N a hair above the faint-limit star's drops it (and only it)
    r = _run("scatterCluster", "--outputFileBase", base, "--brightLimit", "12", "--faintLimit", "20", "--relevantFilt", "1",
             "--limitS2N", repr(s2n_limit + 2e-9), "--sigmaFloor", repr(floor), "--sigmaAtLimit", repr(at_limit), "--scatterSeed", str(seed),
             env=env)
    assert r.returncode == 0, r.stderr
    ids = [int(ln.split()[0]) for ln in open(base + ".sim.scatter").read().splitlines()[1:]]
    assert ids == [0, 7, 40]
    # the output reads back through the .phot reader
    import ctypes as C
    lib = hostlib.load()
    h, view = C.c_void_p(), abi.b9_stars()
    buf = C.create_string_buffer(256)
    _run("scatterCluster", "--outputFileBase", base, "--brightLimit", "12", "--faintLimit", "20", "--relevantFilt", "1",
         "--sigmaFloor", repr(floor), "--sigmaAtLimit", repr(at_limit), "--scatterSeed", str(seed), env=env)
    assert lib.b9h_read_phot((base + ".sim.scatter").encode(), -1e300, 1e300, 0, C.byref(h), C.byref(view), buf, 256) == 0, lib.b9h_last_error()
    try:
        assert view.n_stars == 4 and view.n_filt == 3 and buf.value.decode() == "B,V,I"
        np.testing.assert_allclose(np.ctypeslib.as_array(view.obs, shape=(12,)).reshape(4, 3), obs, atol=1e-9)
        np.testing.assert_array_equal(np.ctypeslib.as_array(view.wd_type, shape=(4,)), [0, 0, 1, 0])
    finally:
        lib.b9h_free_phot(h)


def test_sim_settings_defaults_yaml_and_flags(tmp_path):
    d = hostlib.sim_settings("simCluster", [])
    assert d == dict(nStars=100, nFieldStars=0, percentBinary=0, percentDB=0, minMass=0.1, maxMass=8.0, minMassRatio=0,
                     memberPrior=0.9, nPops=1, seed=73)
    y = tmp_path / "b.yaml"
    y.write_text("general:\n  seed: 11\n  white_dwarfs:\n    M_wd_up: 7.0\nsimCluster:\n  nStars: 500\n  percentBinary: 30\n"
                 "  nFieldStars: 20\nscatterCluster:\n  faintLimit: 21.5\n  sigmaFloor: 0.02\n")
    d = hostlib.sim_settings("simCluster", ["--config", str(y)])
    assert (d["nStars"], d["percentBinary"], d["nFieldStars"], d["maxMass"], d["seed"]) == (500, 30, 20, 7.0, 11)
    d = hostlib.sim_settings("simCluster", ["--config", str(y), "--nStars", "42", "--maxMass", "5.5", "--percentDB", "10", "--nPops", "2"])
    assert (d["nStars"], d["maxMass"], d["percentDB"], d["nPops"], d["percentBinary"]) == (42, 5.5, 10, 2, 30)
    s = hostlib.sim_settings("scatterCluster", ["--config", str(y)])
    assert (s["faintLimit"], s["sigmaFloor"], s["sigmaAtLimit"], s["seed"], s["relevantFilt"]) == (21.5, 0.02, 0.1, 12, 0)
    s = hostlib.sim_settings("scatterCluster", ["--config", str(y), "--faintLimit", "19", "--scatterSeed", "5", "--limitS2N", "8"])
    assert (s["faintLimit"], s["seed"], s["limitS2N"]) == (19, 5, 8)
    for args, msg in ((["--percentBinary", "100.5"], "percentBinary"), (["--percentDB", "-1"], "percentDB"),
                      (["--minMass", "2", "--maxMass", "2"], "minMass must be smaller"), (["--nPops", "3"], "nPops"),
                      (["--minMassRatio", "1"], "minMassRatio"), (["--nStars", "0"], "nStars")):
        with pytest.raises(hostlib.HostError, match=msg):
            hostlib.sim_settings("simCluster", args)
    for args, msg in ((["--brightLimit", "20", "--faintLimit", "20"], "brightLimit"), (["--sigmaFloor", "0", "--sigmaAtLimit", "0"], "sigmaFloor")):
        with pytest.raises(hostlib.HostError, match=msg):
            hostlib.sim_settings("scatterCluster", args)
    with pytest.raises(hostlib.HostError, match="unknown flag"):
        hostlib.sim_settings("simCluster", ["--nStar", "3"])


def test_simcluster_refuses_bad_settings_before_any_gpu_work(tmp_path):
    """Bad values, and two populations on a pack without a helium axis, fail before a context is created (so also here)."""
    pack_d = synth.make_pack("dsed", 4, n_feh=3, n_age=4, n_eep=30)
    root = synth.write_models_dir(pack_d, str(tmp_path / "models"))
    common = ["--modelDirectory", root, "--msRgbModel", "dsed", "--outputFileBase", str(tmp_path / "run")]
    r = _run("simCluster", *common, "--percentBinary", "150")
    assert r.returncode != 0 and "percentBinary must lie in [0, 100]" in r.stderr
    r = _run("simCluster", *common, "--minMass", "3", "--maxMass", "1")
    assert r.returncode != 0 and "minMass must be smaller" in r.stderr
    r = _run("simCluster", *common, "--nPops", "2")
    assert r.returncode != 0 and "helium axis" in r.stderr
    assert not os.path.exists(str(tmp_path / "run.sim.out"))
