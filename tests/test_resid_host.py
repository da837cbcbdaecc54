"""CPU tests of the photResiduals host side and of the checkers themselves: the comparators of tests/resid_check.py must
accept the reference (tests/resid_ref.py) and reject six mutated references, each on a case where the reference itself shows
that the mutation matters; the reference's own sanity; b9h_resid_table / b9h_filter_resid_table against the numpy
restatements; the two files; photResiduals' flags and YAML keys."""
import numpy as np
import pytest

import moments_ref as mr
import resid_check as rc
import resid_ref as rr
from base_amd import abi, hostlib, synth
from conftest import build_problem

N_NODES = 712                                            # case 1 of tests/test_gpu_moments.py: 2 populations x 89 intervals x 2 x 2


@pytest.fixture(scope="module")
def host():
    from base_amd import host_build
    host_build.build_host()
    return hostlib.load()


@pytest.fixture(scope="module", autouse=True)
def the_call_exists():
    """Everything here checks b9_phot_resid's statement or its host side: none of it stands without the call."""
    assert "b9_phot_resid" in abi.ABI_SYMBOLS and "b9h_resid_table" in hostlib.HOST_SYMBOLS


@pytest.fixture(scope="module")
def case1():
    pack_d, cl, pack, stars, priors, _ = build_problem("dsed", 5, n_stars=130, wd_frac=0.1, n_y=3, n_pops=2, seed=12)
    cl = dict(cl)
    cl["sigma"] = np.array(cl["sigma"], dtype=np.float64)
    cl["sigma"][::7, 2] = -1.0                            # every seventh star was not observed in the third filter
    rows = synth.walker_params(cl["truth"], 3, seed=3, scale=0.3)
    rows[:, abi.P_LAMBDA] = 0.3                          # (at 0.5 leaving the population weight out changes nothing)
    nodes = rr.nodes_of_rows(pack_d, cl, rows, 2, 2, 2)
    return pack_d, cl, rows, nodes


@pytest.fixture(scope="module")
def truth(case1):
    pack_d, cl, rows, nodes = case1
    return rr.reference(pack_d, cl, rows, 2, 2, 2, nodes)


def rejects(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


MUTATIONS = [
    ("pivot left out", dict(no_pivot=True), True),
    ("second moment built from d instead of d^2", dict(second_from_d=True), True),
    ("log lambda_k dropped", dict(drop_pop_weight=True), True),
    ("membership weight dropped", dict(drop_membership=True), True),
    ("unused filters counted in the row sums", dict(count_unused=True), False),
    ("sign of z flipped", dict(flip_z=True), False),
]


@pytest.mark.parametrize("what,mutation,in_star", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_comparators_reject_mutated_references(case1, truth, what, mutation, in_star):
    pack_d, cl, rows, nodes = case1
    nf = pack_d["n_filt"]
    want_star, want_rows, x, bound, absx = truth
    a_star, a_rows = rc.star_atol(bound, absx, N_NODES), rc.row_atol(bound, absx, cl["sigma"], N_NODES)
    # the reference passes its own comparators, and so does a copy perturbed at a tenth of the tolerance
    for fs, fr in ((1.0, 1.0), (1 + 1e-10, 1 - 1e-10)):
        rc.assert_star_resid(want_star * np.r_[1.0, np.full(want_star.shape[1] - 1, fs)], want_star, a_star)
        rc.assert_row_resid(want_rows * fr, want_rows, a_rows)
        rc.assert_variances(want_star, want_star, cl)
    got_star, got_rows, *_ = rr.reference(pack_d, cl, rows, 2, 2, 2, nodes, **mutation)
    # the mutation matters on this case: the reference itself says so, far above every tolerance
    d_star, d_rows = rc.largest_rel(got_star, want_star, 1e-3), rc.largest_rel(got_rows, want_rows, 1e-3)
    print(f"{what}: largest relative difference star_resid {d_star:.3g}, row_resid {d_rows:.3g}")
    assert d_rows > 1e-3 and (d_star > 1e-3) == in_star
    assert rejects(rc.assert_row_resid, got_rows, want_rows, a_rows)
    want_ft, got_ft = rr.filter_table(want_rows, nf), rr.filter_table(got_rows, nf)
    rc.assert_filter_table(want_ft, want_ft)
    assert rejects(rc.assert_filter_table, got_ft, want_ft)
    if in_star:
        assert rejects(rc.assert_star_resid, got_star, want_star, a_star)
        want_t = rr.star_table(want_star, cl)
        got_t = rr.star_table(got_star, cl)               # (read as the real call's accumulator would be)
        rc.assert_star_table(want_t, want_t, want_star, cl)
        assert rejects(rc.assert_star_table, got_t, want_t, want_star, cl)
    if "second_from_d" in mutation:
        assert rejects(rc.assert_variances, got_star, want_star, cl)


def test_reference_sanity(case1, truth):
    pack_d, cl, rows, nodes = case1
    nf = pack_d["n_filt"]
    star, rws, x, bound, absx = truth
    live, spread, unused, wd = rc.non_vacuity(star, cl)
    print(f"{live} live stars, {spread} with predSd > 1e-6 somewhere, {unused} with an unused filter, {wd} live WD-stage stars")
    assert live >= 90 and spread == live and unused >= 18 and wd >= 1
    # E[d^2] >= E[d]^2 for every star and filter
    m1, m2, var = rr.star_moments_of(star, cl)
    assert np.all(var >= -1e-12 * m2)
    # the row sums equal the per-star sums re-added in numpy (pairwise sums there, sequential here: both within n eps of the
    # sum of the magnitudes, so rtol 1e-12 of sum |terms| -- for R and D, whose terms cancel, that sum is not the entry)
    sig = np.asarray(cl["sigma"])
    np.testing.assert_allclose(rws[:, 0], x[:, :, 1].sum(axis=1), rtol=1e-12)
    for f in range(nf):
        u = sig[:, f] > 0
        r_terms, d_terms = x[:, u, 2 + 2 * f] / sig[u, f], x[:, u, 2 + 2 * f] / sig[u, f] ** 2
        np.testing.assert_allclose(rws[:, 1 + 5 * f], x[:, u, 1].sum(axis=1), rtol=1e-12)
        assert np.all(np.abs(rws[:, 2 + 5 * f] + r_terms.sum(axis=1)) <= 1e-12 * np.abs(r_terms).sum(axis=1))
        np.testing.assert_allclose(rws[:, 3 + 5 * f], (x[:, u, 3 + 2 * f] / sig[u, f] ** 2).sum(axis=1), rtol=1e-12)
        np.testing.assert_allclose(rws[:, 4 + 5 * f], (x[:, u, 1] / sig[u, f] ** 2).sum(axis=1), rtol=1e-12)
        assert np.all(np.abs(rws[:, 5 + 5 * f] + d_terms.sum(axis=1)) <= 1e-12 * np.abs(d_terms).sum(axis=1))
    # a row outside the grid adds nothing
    out = rows[0].copy(); out[abi.P_LOGAGE] = pack_d["log_age"][-1] + 1.0
    assert np.all(rr.increments(pack_d, cl, out, 2, 2, 2)[0] == 0)


def test_reference_sharpened_star():
    """A star whose sigma is made 50 x sharper around a node's own forward_mags: predMag is that node's magnitudes, predSd ~ 0."""
    pack_d, cl, pack, stars, priors, _ = build_problem("parsec", 4, n_stars=20, wd_frac=0.0, seed=12)
    cl = dict(cl)
    par = np.array(cl["truth"], dtype=np.float64)
    nodes = mr.star_nodes(pack_d, cl, par, 1, 2, 2)
    i = 3
    t, m, q, k = nodes[i]
    node = int(np.argmax(t))
    mags = synth.forward_mags(pack_d, par, m[node:node + 1], q[node:node + 1])[0]
    cl["obs"] = np.array(cl["obs"], dtype=np.float64); cl["sigma"] = np.array(cl["sigma"], dtype=np.float64)
    cl["obs"][i] = mags
    cl["sigma"][i] = np.abs(cl["sigma"][i]) / 50.0
    x, _, _ = rr.increments(pack_d, cl, par, 1, 2, 2)
    tab = rr.star_table(x, cl)
    np.testing.assert_allclose(tab[i, 2::4], mags, rtol=0, atol=1e-9)
    assert np.all(tab[i, 3::4] < 1e-4) and np.all(np.abs(tab[i, 4::4]) < 1e-9)


def test_reference_two_populations_with_lambda_one():
    """Two populations with lambda -> 1 equal one population."""
    pack_d, cl, pack, stars, priors, _ = build_problem("dsed", 4, n_stars=30, wd_frac=0.1, n_y=3, n_pops=2, seed=12)
    par = np.array(cl["truth"], dtype=np.float64)
    par[abi.P_LAMBDA] = 1.0 - 1e-15
    two, _, _ = rr.increments(pack_d, cl, par, 2, 2, 2)
    one, _, _ = rr.increments(pack_d, cl, par, 1, 2, 2)
    assert (one[:, 1] > 0).sum() >= 20
    np.testing.assert_allclose(two, one, rtol=1e-9, atol=1e-12)


# ---- the host tables --------------------------------------------------------------------------------------------------------
def example(n, nf, n_rows, seed=4):
    rng = np.random.default_rng(seed)
    obs = rng.uniform(12, 22, (n, nf))
    sigma = rng.uniform(0.01, 0.1, (n, nf))
    sigma[rng.uniform(size=(n, nf)) < 0.2] = -1.0
    cl = dict(obs=obs, sigma=sigma, stage=np.full(n, abi.STAGE_MSRG))
    acc = np.zeros((n, 2 + 2 * nf))
    acc[:, 0] = n_rows
    acc[:, 1] = rng.uniform(0.1, 1.0, n) * n_rows
    d = rng.normal(0, 0.05, (n, nf))
    acc[:, 2::2] = acc[:, 1:2] * d
    acc[:, 3::2] = acc[:, 1:2] * (d ** 2 + rng.uniform(0, 0.01, (n, nf)))
    return cl, acc


def test_resid_table(host):
    cl, acc = example(40, 5, 12)
    acc[4, 1:] = 0.0                                     # counted, no membership weight (acc1 == 0): every derived value 0
    acc[9] = 0.0                                         # never counted
    got, want = hostlib.resid_table(acc, cl["obs"], cl["sigma"]), rr.star_table(acc, cl)
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-300)
    assert got[4, 0] == 12 and np.all(got[4, 1:] == 0) and np.all(got[9] == 0)
    unused = ~(cl["sigma"] > 0)
    assert unused.sum() >= 20 and np.all(got[:, 4::4][unused] == 0) and np.all(got[:, 5::4][unused] == 0)
    live = acc[:, 1] > 0
    assert np.all(got[live][:, 2::4][unused[live]] != 0)           # an unused filter still has its predicted magnitude


def test_filter_resid_table(host):
    rng = np.random.default_rng(7)
    nf, n_rows = 4, 37
    rr_ = np.zeros((n_rows, 1 + 5 * nf))
    rr_[:, 0] = 100
    for f in range(nf):
        N = rng.uniform(50, 90, n_rows)
        rr_[:, 1 + 5 * f], rr_[:, 2 + 5 * f], rr_[:, 3 + 5 * f] = N, N * rng.normal(0, 1, n_rows), N * rng.gamma(2, 1, n_rows)
        rr_[:, 4 + 5 * f] = N * 400.0
        rr_[:, 5 + 5 * f] = rr_[:, 4 + 5 * f] * rng.normal(0, 0.02, n_rows)
    rr_[3] = 0.0                                         # a row outside the grid stays out of the statistics
    rr_[:, 1 + 5 * 2:6 + 5 * 2] = 0.0                    # a filter no star observed: N_f = 0 in every row
    got, want = hostlib.filter_resid_table(rr_, nf), rr.filter_table(rr_, nf)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-300)
    assert got[0, 0] == n_rows - 1 and np.all(got[2] == 0)
    assert np.all(got[[0, 1, 3], 3] <= got[[0, 1, 3], 4]) and np.all(got[[0, 1, 3], 4] <= got[[0, 1, 3], 5])
    one = hostlib.filter_resid_table(rr_[:1], nf)         # a single-row chain: no spread
    assert np.all(one[[0, 1, 3], 2] == 0) and np.array_equal(one[:, 3], one[:, 5])


def test_files_round_trip(host, tmp_path):
    cl, acc = example(9, 3, 5)
    acc[4, 1:] = 0.0
    tab = hostlib.resid_table(acc, cl["obs"], cl["sigma"])
    ids = [f"s{5 * i % 9:02d}" for i in range(9)]
    filters = ["U", "B", "V"]
    path = str(tmp_path / "x.photResid")
    hostlib.write_phot_resid(path, ids, filters, tab)
    got_ids, cols, got = hostlib.read_phot_resid(path)
    assert got_ids == ids and cols == ["rows", "member"] + [f"{f}_{c}" for f in filters for c in hostlib.RESID_STAR_COLUMNS]
    assert np.array_equal(got, tab)                      # 17 significant digits: the bits come back
    ft = hostlib.filter_resid_table(np.random.default_rng(1).uniform(0.5, 2.0, (6, 16)), 3)
    path = str(tmp_path / "x.filterResid")
    hostlib.write_filter_resid(path, filters, ft)
    names, cols, got = hostlib.read_filter_resid(path)
    assert names == filters and cols == list(hostlib.FILTER_RESID_COLUMNS) == list(rr.FILTER_COLUMNS)
    assert np.array_equal(got, ft)


# ---- flags and YAML -----------------------------------------------------------------------------------------------------------
def test_flags_and_yaml_parse(host, tmp_path):
    assert hostlib.phot_resid_settings([]) == dict(margIsoIncrem=4, nMassRatios=4, nPops=1, perStar=0)
    d = hostlib.phot_resid_settings(["--perStar", "--nPops", "2", "--margIsoIncrem", "2", "--nMassRatios=3"])
    assert d == dict(margIsoIncrem=2, nMassRatios=3, nPops=2, perStar=1)
    y = tmp_path / "pr.yaml"
    y.write_text("sampleMass:\n  margIsoIncrem: 6\n  nMassRatios: 5\nmassFunction:\n  perStar: 1\nsimCluster:\n  nPops: 2\n"
                 "photResiduals:\n  nMassRatios: 7\n")
    d = hostlib.phot_resid_settings(["--config", str(y)])                    # sampleMass's grid is the default; other programs' keys are not read
    assert d == dict(margIsoIncrem=6, nMassRatios=7, nPops=1, perStar=0)
    y.write_text("photResiduals:\n  margIsoIncrem: 3\n  nMassRatios: 2\n  nPops: 2\n  perStar: 1\n")
    assert hostlib.phot_resid_settings(["--config", str(y)]) == dict(margIsoIncrem=3, nMassRatios=2, nPops=2, perStar=1)
    assert hostlib.phot_resid_settings(["--config", str(y), "--perStar=0", "--nPops=1"]) == dict(margIsoIncrem=3, nMassRatios=2, nPops=1, perStar=0)
    for bad in (["--nPops", "3"], ["--margIsoIncrem", "0"], ["--nMassRatios", "0"]):
        with pytest.raises(hostlib.HostError):
            hostlib.phot_resid_settings(bad)


def test_short_and_long_flags(host):
    """--perStar / --nPops are photResiduals' own spellings of --photResidualsPerStar / --photResidualsNPops: both give the same
    settings, on this program's command line only.  The shared table gives --perStar to massFunction: the long spelling sets the
    program's key and no other, and the program reads the short one as the long one."""
    from cli_util import settings_dump
    short = hostlib.phot_resid_settings(["--perStar", "--nPops", "2"])
    long_ = hostlib.phot_resid_settings(["--photResidualsPerStar=1", "--photResidualsNPops", "2"])
    assert short == long_ == dict(margIsoIncrem=4, nMassRatios=4, nPops=2, perStar=1)
    assert hostlib.phot_resid_settings(["--perStar=1", "--nPops=2"]) == short
    assert hostlib.phot_resid_settings(["--perStar=0"])["perStar"] == 0
    assert settings_dump(["--photResidualsPerStar=1", "--photResidualsNPops", "2"]) == {"photResiduals.perStar": "1", "photResiduals.nPops": "2"}
    assert settings_dump(["--perStar", "--nPops", "2"]) == {"massFunction.perStar": "1", "simCluster.nPops": "2"}
    for bad in (["--perStar", "0"], ["--perStar", "0", "--nPops", "2"]):
        with pytest.raises(hostlib.HostError, match="unexpected argument '0'"):
            hostlib.phot_resid_settings(bad)
    # another program's short flags: known to the shared table -> accepted, and nothing of photResiduals' changes; else refused
    assert hostlib.phot_resid_settings(["--quantity", "system", "--minMass", "0.5"]) == hostlib.phot_resid_settings([])
    with pytest.raises(hostlib.HostError):
        hostlib.phot_resid_settings(["--perRow"])                       # modelScore's
