"""CPU tests of b9_filter_loo's statement and of the checkers themselves: the non-vacuity of the two fixtures (asserted on the
reference before anything else), the comparators of tests/loo_check.py accepting the reference (tests/loo_ref.py) and
rejecting six mutated references, the reference's own sanity, the zero-point case, and the binding tables."""
import functools

import numpy as np
import pytest

import loo_check as lc
import loo_ref as lr
import moments_ref as mr
import resid_ref as rr
import test_gpu_moments as tm
from base_amd import abi
from conftest import build_problem

K = Q = 2
FIXTURES = {      # name: (build_problem arguments, populations, N_nodes = pops x 89 intervals x 2 x 2, the figures measured: shifted, promoted, revived)
    "parsec4": (("parsec", 4), dict(n_stars=70, wd_frac=0.1, seed=12), 1, 356, (137, 4, 137)),
    "dsed5": (("dsed", 5), dict(n_stars=70, wd_frac=0.1, n_y=3, n_pops=2, seed=12), 2, 712, (191, 15, 334)),
}


@pytest.fixture(scope="module", autouse=True)
def the_call_exists():
    """Everything here checks b9_filter_loo's statement: none of it stands without the call."""
    assert "b9_filter_loo" in abi.ABI_SYMBOLS


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(pack_d, cl, row, nodes, n_pops, n_nodes) of a non-vacuity fixture: the first of test_gpu_moments.rows_for's rows."""
    args, kw, n_pops, n_nodes, _ = FIXTURES[name]
    pack_d, cl, _, _, _, _ = build_problem(*args, **kw)
    row = tm.rows_for(pack_d, cl, n_pops)[0]
    nodes = mr.star_nodes(pack_d, cl, row, n_pops, K, Q)
    assert n_nodes == tm.n_nodes_of(pack_d, n_pops, K, Q)
    return pack_d, cl, row, nodes, n_pops, n_nodes


@functools.lru_cache(maxsize=None)
def truth(name):
    pack_d, cl, row, nodes, n_pops, _ = fixture(name)
    return lr.reference(pack_d, cl, row[None, :], n_pops, K, Q, [nodes])


def rejects(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("name", list(FIXTURES))
def test_the_fixtures_are_not_vacuous(name):
    """The leave-outs differ from the in-sample sums in all three ways the kernels must handle: the prediction shifts, the
    largest leave-out term is promoted far above the largest full term, and nodes the full-data pruning drops are live in a
    leave-out.  Measured: parsec 4: 137 of 278 pairs shift by more than 1e-3 mag (at most 0.11), 4 promoted (by up to 11 734
    e-folds), 137 nodes revived; dsed 5: 191 of 350 (1.19 mag), 15 (81 742), 334."""
    pack_d, cl, row, nodes, n_pops, _ = fixture(name)
    nv = lr.non_vacuity(pack_d, cl, row, n_pops, K, Q, nodes)
    print(f"{name}: {nv['shifted']} of {nv['pairs']} pairs shift by more than 1e-3 mag (largest {nv['max_shift']:.3g}), {nv['promoted']} promoted by more "
          f"than 40 e-folds (largest {nv['max_promotion']:.6g}), {nv['revived']} nodes live only when left out")
    assert nv["shifted"] >= 100 and nv["promoted"] >= 3 and nv["revived"] >= 100


MUTATIONS = [
    ("in-sample weights", dict(in_sample=True), True, "parsec4"),
    ("leave-out sums under the full-data pruning", dict(full_pruning=True), True, "dsed5-members"),
    ("l_f without -log(sigma sqrt(2 pi))", dict(no_norm=True), True, "parsec4"),
    ("g_f without the 1/2", dict(no_half=True), True, "parsec4"),
    ("full-data population weights for every leave-out", dict(full_pop_weights=True), True, "dsed5"),
    ("unused filters counted in the row sums", dict(count_unused=True), False, "dsed5"),
]


@pytest.mark.parametrize("what,mutation,in_star,name", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_comparators_reject_mutated_references(what, mutation, in_star, name):
    name, members = name.split("-")[0], name.endswith("-members")
    pack_d, cl, row, nodes, n_pops, n_nodes = fixture(name)
    if "count_unused" in mutation or members:
        cl = dict(cl)
        if members:                                          # (the promoted pairs are outliers: with a field alternative their membership is ~0)
            cl["clust_prior"] = np.ones(len(cl["mass1"]))
        else:                                                # every seventh star was not observed in the third filter
            cl["sigma"] = np.array(cl["sigma"], dtype=np.float64)
            cl["sigma"][::7, 2] = -1.0
        want_star, want_rows, x, bound, absx = lr.reference(pack_d, cl, row[None, :], n_pops, K, Q, [nodes])
    else:
        want_star, want_rows, x, bound, absx = truth(name)
    a_star, a_rows = lc.star_atol(bound, absx, n_nodes), lc.row_atol(bound, absx, cl["sigma"], n_nodes)
    # the reference passes its own comparators, and so does a copy perturbed at a tenth of the tolerance
    for fs, fr in ((1.0, 1.0), (1 + 1e-10, 1 - 1e-10)):
        lc.assert_star_loo(want_star * np.r_[1.0, np.full(want_star.shape[1] - 1, fs)], want_star, a_star)
        lc.assert_row_loo(want_rows * fr, want_rows, a_rows)
        lc.assert_variances(want_star, want_star)
    got_star, got_rows, *_ = lr.reference(pack_d, cl, row[None, :], n_pops, K, Q, [nodes], **mutation)
    d_star, d_rows = lc.largest_rel(got_star, want_star, 1e-3), lc.largest_rel(got_rows, want_rows, 1e-3)
    print(f"{what}: largest relative difference star_loo {d_star:.3g}, row_loo {d_rows:.3g}")
    assert d_rows > 1e-3 and (d_star > 1e-3) == in_star
    assert rejects(lc.assert_row_loo, got_rows, want_rows, a_rows)
    nf = pack_d["n_filt"]
    want_ft = lr.filter_table(want_rows, nf)
    lc.assert_filter_table(want_ft, want_ft)
    assert rejects(lc.assert_filter_table, lr.filter_table(got_rows, nf), want_ft)
    if in_star:
        assert rejects(lc.assert_star_loo, got_star, want_star, a_star)
        want_t = lr.star_table(want_star, cl)
        lc.assert_star_table(want_t, want_t, want_star, cl)
        assert rejects(lc.assert_star_table, lr.star_table(got_star, cl), want_t, want_star, cl)


@pytest.mark.parametrize("name", list(FIXTURES))
def test_reference_sanity(name):
    pack_d, cl, row, nodes, n_pops, _ = fixture(name)
    nf = pack_d["n_filt"]
    star, rws, x, bound, absx = truth(name)
    sig = np.asarray(cl["sigma"], dtype=np.float64)
    # ROWS and MEMBER are resid_ref's; E[d^2] >= E[d]^2 under every leave-out's weights
    xr = rr.increments(pack_d, cl, row, n_pops, K, Q, nodes)[0]
    assert np.array_equal(star[:, :2], xr[:, :2]) and (star[:, 1] > 0).sum() >= 60
    m1, m2, var = lc.star_moments_of(star)
    assert np.all(var >= -1e-12 * m2)
    # leaving a filter out can only raise the log-sum: l_f + log(sigma sqrt(2 pi)) = L - L^f <= 0, and the observation's density
    # under the other filters' prediction is no sharper than the filter's own error allows
    live = star[:, 1] > 0
    lsn = np.where(sig > 0, np.log(np.where(sig > 0, sig, 1.0)) + lr.LOG_SQRT_2PI, 0.0)
    lpd = star[live, 4::3] / star[live, 1:2]
    assert np.all(lpd + lsn[live] <= 1e-9) and np.all(lpd[~(sig[live] > 0)] == 0)
    # an unused filter's two sums are the in-sample ones
    cl2 = dict(cl)
    cl2["sigma"] = np.array(sig)
    cl2["sigma"][::5, 1] = -1.0
    x2 = lr.increments(pack_d, cl2, row, n_pops, K, Q)[0]
    r2 = rr.increments(pack_d, cl2, row, n_pops, K, Q)[0]
    sel = np.flatnonzero(x2[::5, 1] > 0) * 5
    assert len(sel) >= 8
    np.testing.assert_allclose(x2[sel, 2 + 3 * 1], r2[sel, 2 + 2 * 1], rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(x2[sel, 3 + 3 * 1], r2[sel, 3 + 2 * 1], rtol=1e-12, atol=1e-300)
    assert np.all(x2[sel, 4 + 3 * 1] == 0)
    # the row sums equal the per-star sums re-added in numpy
    np.testing.assert_allclose(rws[:, 0], x[:, :, 1].sum(axis=1), rtol=1e-12)
    for f in range(nf):
        u = sig[:, f] > 0
        np.testing.assert_allclose(rws[:, 1 + 6 * f], x[:, u, 1].sum(axis=1), rtol=1e-12)
        np.testing.assert_allclose(rws[:, 3 + 6 * f], (x[:, u, 3 + 3 * f] / sig[u, f] ** 2).sum(axis=1), rtol=1e-12)
        np.testing.assert_allclose(rws[:, 6 + 6 * f], x[:, u, 4 + 3 * f].sum(axis=1), rtol=1e-12)
    # a row outside the grid adds nothing
    out = row.copy(); out[abi.P_LOGAGE] = pack_d["log_age"][-1] + 1.0
    assert np.all(lr.increments(pack_d, cl, out, n_pops, K, Q)[0] == 0)


def test_zero_point_case():
    """A simulated catalogue with +0.05 mag added to one band, the row at the truth.  The in-sample offset D / W of that band
    (resid_ref) is shrunk towards zero -- the band helped choose the weights -- and part of the error is smeared over the other
    bands; the leave-out offset is closer to +0.05, and no other band's leave-out offset exceeds the shifted band's.
    Measured (parsec, 8 filters, 150 stars, band 2): in-sample 0.0441, leave-out 0.0483; the largest other band -0.0127."""
    b, shift = 2, 0.05
    pack_d, cl, _, _, _, _ = build_problem("parsec", 8, n_stars=150, wd_frac=0.0, seed=12)
    cl = dict(cl)
    cl["obs"] = np.array(cl["obs"], dtype=np.float64)
    cl["obs"][:, b] += shift
    row = np.array(cl["truth"], dtype=np.float64)
    nodes = mr.star_nodes(pack_d, cl, row, 1, K, Q)
    _, loo_rows, *_ = lr.reference(pack_d, cl, row[None, :], 1, K, Q, [nodes])
    _, in_rows, *_ = rr.reference(pack_d, cl, row[None, :], 1, K, Q, [nodes])
    nf = pack_d["n_filt"]
    loo = np.array([loo_rows[0, 5 + 6 * f] / loo_rows[0, 4 + 6 * f] for f in range(nf)])
    ins = np.array([in_rows[0, 5 + 5 * f] / in_rows[0, 4 + 5 * f] for f in range(nf)])
    print(f"band {b}: in-sample offset {ins[b]:.4f}, leave-out offset {loo[b]:.4f}; leave-out offsets of all bands {np.round(loo, 4)}")
    assert abs(loo[b] - shift) < abs(ins[b] - shift)
    assert np.all(np.abs(np.delete(loo, b)) <= abs(loo[b]))


# ---- the host tables --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    from base_amd import host_build, hostlib
    host_build.build_host()
    assert "b9h_loo_table" in hostlib.HOST_SYMBOLS
    return hostlib.load()


def example(n, nf, n_rows, seed=4):
    rng = np.random.default_rng(seed)
    obs = rng.uniform(12, 22, (n, nf))
    sigma = rng.uniform(0.01, 0.1, (n, nf))
    sigma[rng.uniform(size=(n, nf)) < 0.2] = -1.0
    cl = dict(obs=obs, sigma=sigma, stage=np.full(n, abi.STAGE_MSRG))
    acc = np.zeros((n, 2 + 3 * nf))
    acc[:, 0] = n_rows
    acc[:, 1] = rng.uniform(0.1, 1.0, n) * n_rows
    d = rng.normal(0, 0.05, (n, nf))
    acc[:, 2::3] = acc[:, 1:2] * d
    acc[:, 3::3] = acc[:, 1:2] * (d ** 2 + rng.uniform(0, 0.01, (n, nf)))
    acc[:, 4::3] = np.where(sigma > 0, acc[:, 1:2] * rng.normal(1.0, 2.0, (n, nf)), 0.0)
    return cl, acc


def test_loo_table(host):
    from base_amd import hostlib
    cl, acc = example(40, 5, 12)
    acc[4, 1:] = 0.0                                     # counted, no membership weight (acc1 == 0): every derived value 0
    acc[9] = 0.0                                         # never counted
    got, want = hostlib.loo_table(acc, cl["obs"], cl["sigma"]), lr.star_table(acc, cl)
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-300)
    assert got[4, 0] == 12 and np.all(got[4, 1:] == 0) and np.all(got[9] == 0)
    unused = ~(cl["sigma"] > 0)
    assert unused.sum() >= 20 and all(np.all(got[:, c::5][unused] == 0) for c in (4, 5, 6))
    live = acc[:, 1] > 0
    assert np.all(got[live][:, 2::5][unused[live]] != 0)           # an unused filter still has its predicted magnitude
    # the predictive z: the residual over the observation's and the prediction's spread together
    i, f = np.argwhere(~unused & live[:, None])[0]
    assert got[i, 5 + 5 * f] == got[i, 4 + 5 * f] / np.sqrt(cl["sigma"][i, f] ** 2 + got[i, 3 + 5 * f] ** 2)


def test_filter_loo_table(host):
    from base_amd import hostlib
    rng = np.random.default_rng(7)
    nf, n_rows = 4, 37
    rl = np.zeros((n_rows, 1 + 6 * nf))
    rl[:, 0] = 100
    for f in range(nf):
        N = rng.uniform(50, 90, n_rows)
        rl[:, 1 + 6 * f], rl[:, 2 + 6 * f], rl[:, 3 + 6 * f] = N, N * rng.normal(0, 1, n_rows), N * rng.gamma(2, 1, n_rows)
        rl[:, 4 + 6 * f] = N * 400.0
        rl[:, 5 + 6 * f] = rl[:, 4 + 6 * f] * rng.normal(0, 0.02, n_rows)
        rl[:, 6 + 6 * f] = N * rng.normal(1.5, 0.3, n_rows)
    rl[3] = 0.0                                          # a row outside the grid stays out of the statistics
    rl[:, 1 + 6 * 2:7 + 6 * 2] = 0.0                     # a filter no star observed: N_f = 0 in every row
    got, want = hostlib.filter_loo_table(rl, nf), lr.filter_table(rl, nf)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-300)
    assert got[0, 0] == n_rows - 1 and np.all(got[2] == 0)
    assert np.all(got[[0, 1, 3], 18] <= got[[0, 1, 3], 19]) and np.all(got[[0, 1, 3], 19] <= got[[0, 1, 3], 20])
    one = hostlib.filter_loo_table(rl[:1], nf)           # a single-row chain: no spread
    assert np.all(one[[0, 1, 3], 17] == 0) and np.array_equal(one[:, 18], one[:, 20])


def test_files_round_trip(host, tmp_path):
    from base_amd import hostlib
    cl, acc = example(9, 3, 5)
    acc[4, 1:] = 0.0
    tab = hostlib.loo_table(acc, cl["obs"], cl["sigma"])
    ids = [f"s{5 * i % 9:02d}" for i in range(9)]
    filters = ["U", "B", "V"]
    path = str(tmp_path / "x.starFilterCheck")
    hostlib.write_star_filter_check(path, ids, filters, tab)
    got_ids, cols, got = hostlib.read_star_filter_check(path)
    assert got_ids == ids and cols == ["rows", "member"] + [f"{f}_{c}" for f in filters for c in hostlib.LOO_STAR_COLUMNS]
    assert hostlib.LOO_STAR_COLUMNS == lr.STAR_COLUMNS
    assert np.array_equal(got, tab)                      # 17 significant digits: the bits come back
    ft = hostlib.filter_loo_table(np.random.default_rng(1).uniform(0.5, 2.0, (6, 19)), 3)
    path = str(tmp_path / "x.filterCheck")
    hostlib.write_filter_check(path, filters, ft)
    names, cols, got = hostlib.read_filter_check(path)
    assert names == filters and cols == list(hostlib.FILTER_CHECK_COLUMNS) == list(lr.FILTER_COLUMNS)
    assert np.array_equal(got, ft)


def test_flags_and_yaml_parse(host, tmp_path):
    from base_amd import hostlib
    assert hostlib.filter_check_settings([]) == dict(margIsoIncrem=4, nMassRatios=4, nPops=1, perStar=0)
    d = hostlib.filter_check_settings(["--perStar", "--nPops", "2", "--margIsoIncrem", "2", "--nMassRatios=3"])
    assert d == dict(margIsoIncrem=2, nMassRatios=3, nPops=2, perStar=1)
    assert hostlib.filter_check_settings(["--filterCheckPerStar=1", "--filterCheckNPops", "2"]) == dict(margIsoIncrem=4, nMassRatios=4, nPops=2, perStar=1)
    y = tmp_path / "fc.yaml"
    y.write_text("sampleMass:\n  margIsoIncrem: 6\n  nMassRatios: 5\nphotResiduals:\n  perStar: 1\nsimCluster:\n  nPops: 2\n"
                 "filterCheck:\n  nMassRatios: 7\n")
    d = hostlib.filter_check_settings(["--config", str(y)])                  # sampleMass's grid is the default; other programs' keys are not read
    assert d == dict(margIsoIncrem=6, nMassRatios=7, nPops=1, perStar=0)
    y.write_text("filterCheck:\n  margIsoIncrem: 3\n  nMassRatios: 2\n  nPops: 2\n  perStar: 1\n")
    assert hostlib.filter_check_settings(["--config", str(y)]) == dict(margIsoIncrem=3, nMassRatios=2, nPops=2, perStar=1)
    assert hostlib.filter_check_settings(["--config", str(y), "--perStar=0", "--nPops=1"]) == dict(margIsoIncrem=3, nMassRatios=2, nPops=1, perStar=0)
    for bad in (["--nPops", "3"], ["--margIsoIncrem", "0"], ["--nMassRatios", "0"]):
        with pytest.raises(hostlib.HostError):
            hostlib.filter_check_settings(bad)
