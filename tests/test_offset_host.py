"""CPU tests of b9_star_offset's statement and of the checkers themselves: the non-vacuity of the two fixtures (asserted on the
reference before anything else), the comparators of tests/offset_check.py accepting the reference (tests/offset_ref.py) and
rejecting eight mutated references, the exact power-of-two scaling, the paired injection, the tie to filterCheck's leave-outs,
and the binding tables, files, directions and settings."""
import functools

import numpy as np
import pytest

import loo_check as lc
import loo_ref as lr
import moments_ref as mr
import offset_check as oc
import offset_ref as of
import resid_ref as rr
import test_filterloo_host as tf
from base_amd import abi

K = Q = 2
TAU = 0.1
FIXTURES = tf.FIXTURES          # parsec4 (70 stars, one population) and dsed5 (70 stars, n_y = 3, two populations), K = Q = 2
MEASURED = {                    # direction absorption: (shifted, promoted, revived); direction distance: revived
    "parsec4": ((66, 3, 737), 1500),
    "dsed5": ((70, 5, 974), 2767),
}


@pytest.fixture(scope="module", autouse=True)
def the_call_exists():
    """Everything here checks b9_star_offset's statement: none of it stands without the call."""
    assert "b9_star_offset" in abi.ABI_SYMBOLS


def fixture(name):
    """(pack_d, cl, row, nodes, n_pops, n_nodes): test_filterloo_host's, the first of test_gpu_moments.rows_for's rows."""
    return tf.fixture(name)


@functools.lru_cache(maxsize=None)
def truth(name, names=("absorption",), tau=TAU):
    pack_d, cl, row, nodes, n_pops, _ = fixture(name)
    ks = of.directions(pack_d, names)
    return of.reference(pack_d, cl, row[None, :], n_pops, K, Q, ks, [tau] * len(ks), [nodes])


def rejects(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("name", list(FIXTURES))
def test_the_fixtures_are_not_vacuous(name):
    """The offset sums differ from the full-data sums in all three ways the kernels must handle: the weights move, the largest
    boosted term is promoted far above the largest full term, and nodes the full-data pruning drops are live in the offset sum.
    Measured, direction absorption: parsec 4: 66 of 70 stars' weights differ by more than 1e-3 in L1, 3 promoted (by up to
    2059 e-folds), 737 nodes revived; dsed 5: 70 of 70, 5 (7020), 974.  Direction distance: 1500 and 2767 nodes revived."""
    pack_d, cl, row, nodes, n_pops, _ = fixture(name)
    nv = of.non_vacuity(pack_d, cl, row, n_pops, K, Q, of.direction(pack_d, "absorption"), TAU, nodes)
    nd = of.non_vacuity(pack_d, cl, row, n_pops, K, Q, of.direction(pack_d, "distance"), TAU, nodes)
    print(f"{name}: absorption: {nv['shifted']} of {nv['stars']} stars' weights differ by more than 1e-3 in L1, {nv['promoted']} promoted by more than "
          f"40 e-folds (largest {nv['max_promotion']:.6g}), {nv['revived']} nodes live only in the offset sum, largest rho {nv['max_rho']:.4f}; "
          f"distance: {nd['revived']} such nodes")
    assert nv["stars"] == 70
    assert nv["shifted"] >= 60 and nv["promoted"] >= 3 and nv["revived"] >= 500 and nd["revived"] >= 500
    assert ((nv["shifted"], nv["promoted"], nv["revived"]), nd["revived"]) == MEASURED[name]


MUTATIONS = [
    ("full-data weights, no boost", dict(no_boost=True), True, "parsec4"),
    ("offset sums under the full-data pruning", dict(full_pruning=True), True, "dsed5-members"),
    ("boost without the 1/2", dict(no_half=True), True, "parsec4"),
    ("V without tau^-2", dict(no_prior=True), True, "parsec4"),
    ("no log1p Occam term", dict(no_occam=True), True, "parsec4"),
    ("full-data population weights", dict(full_pop_weights=True), True, "dsed5"),
    ("M2 without p V", dict(no_pv=True), False, "parsec4"),
    ("stars with C = 0 counted in the row sums", dict(count_zero=True), False, "dsed5-unused"),
]


@pytest.mark.parametrize("what,mutation,in_star,name", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_comparators_reject_mutated_references(what, mutation, in_star, name):
    name, variant = (name.split("-") + [""])[:2]
    pack_d, cl, row, nodes, n_pops, n_nodes = fixture(name)
    names = ("absorption",)
    if variant:
        cl = dict(cl)
        if variant == "members":                             # (the promoted stars are outliers: with a field alternative their membership is ~0)
            cl["clust_prior"] = np.ones(len(cl["mass1"]))
        else:                                                # every seventh star was not observed in the third filter; the direction is that band
            cl["sigma"] = np.array(cl["sigma"], dtype=np.float64)
            cl["sigma"][::7, 2] = -1.0
            names = ("filter:2",)
    ks, taus = of.directions(pack_d, names), [TAU]
    if variant:
        want_star, want_rows, x, bound, absx = of.reference(pack_d, cl, row[None, :], n_pops, K, Q, ks, taus, [nodes])
    else:
        want_star, want_rows, x, bound, absx = truth(name)
    C, V = of.all_cv(cl, ks, taus)
    a_star, a_rows = oc.star_atol(bound, absx, n_nodes), oc.row_atol(bound, absx, C, V, n_nodes)
    # the reference passes its own comparators, and so does a copy perturbed at a tenth of the tolerance
    for fs, fr in ((1.0, 1.0), (1 + 1e-10, 1 - 1e-10)):
        oc.assert_star_off(want_star * np.r_[1.0, np.full(want_star.shape[1] - 1, fs)], want_star, a_star)
        oc.assert_row_off(want_rows * fr, want_rows, a_rows)
    got_star, got_rows, *_ = of.reference(pack_d, cl, row[None, :], n_pops, K, Q, ks, taus, [nodes], **mutation)
    d_star, d_rows = oc.largest_rel(got_star, want_star, 1e-3), oc.largest_rel(got_rows, want_rows, 1e-3)
    print(f"{what}: largest relative difference star_off {d_star:.3g}, row_off {d_rows:.3g}")
    assert d_rows > 1e-3 and (d_star > 1e-3) == in_star
    assert rejects(oc.assert_row_off, got_rows, want_rows, a_rows)
    want_dt = of.dist_table(want_rows, len(ks))
    oc.assert_dist_table(want_dt, want_dt)
    assert rejects(oc.assert_dist_table, of.dist_table(got_rows, len(ks)), want_dt)
    if in_star:
        assert rejects(oc.assert_star_off, got_star, want_star, a_star)
        want_t = of.star_table(want_star, cl, ks, taus)
        oc.assert_star_table(want_t, want_t)
        assert rejects(oc.assert_star_table, of.star_table(got_star, cl, ks, taus), want_t)


@pytest.mark.parametrize("name", list(FIXTURES))
def test_reference_sanity(name):
    pack_d, cl, row, nodes, n_pops, _ = fixture(name)
    names = ("absorption", "distance", "filter:1")
    star, rws, x, bound, absx = truth(name, names)
    ks = of.directions(pack_d, names)
    # ROWS and MEMBER are resid_ref's; E[mu^2] >= E[mu]^2 under every direction's weights; the boost can only raise the log-sum
    xr = rr.increments(pack_d, cl, row, n_pops, K, Q, nodes)[0]
    assert np.array_equal(star[:, :2], xr[:, :2]) and (star[:, 1] > 0).sum() >= 60
    live = star[:, 1] > 0
    m1, m2 = star[live, 2::3] / star[live, 1:2], star[live, 3::3] / star[live, 1:2]
    assert np.all(m2 - m1 ** 2 >= -1e-12 * m2)
    C, V = of.all_cv(cl, ks, [TAU] * 3)
    occ = 0.5 * np.log1p(C * TAU * TAU)
    assert np.all(star[live, 4::3] / star[live, 1:2] + occ[live] >= -1e-9)
    # a direction's columns do not depend on which other directions are in the call
    for j, n in enumerate(names):
        alone = truth(name, (n,))[0]
        assert np.array_equal(alone[:, 2:], star[:, 2 + 3 * j:5 + 3 * j])
    # the row sums equal the per-star sums re-added in numpy
    np.testing.assert_allclose(rws[:, 0], x[:, :, 1].sum(axis=1), rtol=1e-12)
    for j in range(3):
        u = C[:, j] > 0
        np.testing.assert_allclose(rws[:, 1 + 4 * j], x[:, u, 1].sum(axis=1), rtol=1e-12)
        np.testing.assert_allclose(rws[:, 3 + 4 * j], (x[:, u, 3 + 3 * j] + x[:, u, 1] * V[None, u, j]).sum(axis=1), rtol=1e-12)
    # a row outside the grid adds nothing
    out = row.copy(); out[abi.P_LOGAGE] = pack_d["log_age"][-1] + 1.0
    assert np.all(of.increments(pack_d, cl, out, n_pops, K, Q, ks, [TAU] * 3)[0] == 0)


@pytest.mark.parametrize("name", list(FIXTURES))
def test_power_of_two_scaling_is_exact(name):
    """k -> 2 k with tau -> tau / 2 describes the same offset in half units: every x[2 + 3j] halves and every x[3 + 3j] quarters
    exactly, and x[4 + 3j] keeps its bits (every scaling is by a power of two)."""
    pack_d, cl, row, nodes, n_pops, _ = fixture(name)
    ks = of.directions(pack_d, ("absorption", "distance"))
    a = of.increments(pack_d, cl, row, n_pops, K, Q, ks, [TAU, 0.25], nodes)[0]
    b = of.increments(pack_d, cl, row, n_pops, K, Q, 2.0 * ks, [TAU / 2, 0.125], nodes)[0]
    assert (a[:, 2] != 0).sum() >= 60
    assert np.array_equal(b[:, :2], a[:, :2])
    assert np.array_equal(b[:, 2::3], 0.5 * a[:, 2::3]) and np.array_equal(b[:, 3::3], 0.25 * a[:, 3::3]) and np.array_equal(b[:, 4::3], a[:, 4::3])


@pytest.mark.parametrize("tau,lo_hi", [(0.1, (0.082, 0.145)), (0.3, (0.138, 0.149))])
@pytest.mark.parametrize("name", list(FIXTURES))
def test_paired_injection(name, tau, lo_hi):
    """0.15 abs_coeff added to every fifth star's magnitudes: every injected star's E[delta] along `absorption` rises by more
    than 0 and less than 0.15 (measured: 0.082 to 0.145 at tau = 0.1, 0.138 to 0.149 at tau = 0.3, all 14 stars, both
    fixtures), and every other star's values keep their bits."""
    pack_d, cl, row, nodes, n_pops, _ = fixture(name)
    k = of.directions(pack_d, ("absorption",))
    inj = np.arange(0, 70, 5)
    cl2 = dict(cl)
    cl2["obs"] = np.array(cl["obs"], dtype=np.float64)
    cl2["obs"][inj] += 0.15 * k[0][None, :]
    a = of.increments(pack_d, cl, row, n_pops, K, Q, k, [tau], nodes)[0]
    b = of.increments(pack_d, cl2, row, n_pops, K, Q, k, [tau])[0]
    rest = np.setdiff1d(np.arange(70), inj)
    assert np.array_equal(a[rest], b[rest])
    assert np.all(a[inj, 1] > 0) and np.all(b[inj, 1] > 0)
    rise = b[inj, 2] / b[inj, 1] - a[inj, 2] / a[inj, 1]
    print(f"{name} tau {tau}: E[delta] of the {len(inj)} injected stars rises by {rise.min():.4f} to {rise.max():.4f}")
    assert np.all(rise > 0) and np.all(rise < 0.15)
    assert lo_hi[0] - 5e-4 <= rise.min() and rise.max() <= lo_hi[1] + 5e-4


@pytest.mark.parametrize("name", list(FIXTURES))
def test_tie_to_filter_check(name):
    """Direction filter:f with a wide prior frees band f altogether: t' = t + rho g_f against the leave-out's t^f = t + g_f, so
    0 <= (L^f - L) - (L' - L) <= (1 - rho) max_n g_f(n), within the two comparators' tolerances.  Both from the references."""
    pack_d, cl, row, nodes, n_pops, n_nodes = fixture(name)
    nf, tau = pack_d["n_filt"], 100.0
    ks = of.directions(pack_d, [f"filter:{f}" for f in range(min(nf, 4))])
    nd = len(ks)
    off, _, _, ob, oa = of.reference(pack_d, cl, row[None, :], n_pops, K, Q, ks, [tau] * nd, [nodes])
    loo, _, _, lb, la = lr.reference(pack_d, cl, row[None, :], n_pops, K, Q, [nodes])
    tol_off, tol_loo = oc.star_atol(ob, oa, n_nodes), lc.star_atol(lb, la, n_nodes)
    C, V = of.all_cv(cl, ks, [tau] * nd)
    sig = np.asarray(cl["sigma"], dtype=np.float64)
    mags = rr.node_mags(pack_d, cl, row, nodes)
    checked, widest = 0, 0.0
    for i in range(70):
        p = off[i, 1]
        if mags[i] is None or not p > 0:
            continue
        g, _ = lr.leave_out_terms(cl, i, nodes[i][0], mags[i])
        for f in range(nd):
            if not sig[i, f] > 0:
                continue
            lsn = np.log(sig[i, f]) + lr.LOG_SQRT_2PI
            occ = 0.5 * np.log1p(C[i, f] * tau * tau)
            full_out = -(loo[i, 4 + 3 * f] / p + lsn)                        # L^f - L
            boosted = off[i, 4 + 3 * f] / p + occ                            # L' - L
            slack = (1.0 - C[i, f] * V[i, f]) * g[:, f].max()
            tol = (tol_off[i, 4 + 3 * f] + tol_loo[i, 4 + 3 * f] + lc.RTOL * (abs(off[i, 4 + 3 * f]) + abs(loo[i, 4 + 3 * f]))) / p
            assert -tol <= full_out - boosted <= slack + tol
            checked += 1
            widest = max(widest, slack)
    print(f"{name}: {checked} (star, filter) pairs, the widest allowance (1 - rho) max g {widest:.3g}")
    assert checked >= 200


# ---- the host tables --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    from base_amd import host_build, hostlib
    host_build.build_host()
    assert "b9h_offset_table" in hostlib.HOST_SYMBOLS
    return hostlib.load()


def example(n, nf, nd, n_rows, seed=4):
    rng = np.random.default_rng(seed)
    sigma = rng.uniform(0.01, 0.1, (n, nf))
    sigma[rng.uniform(size=(n, nf)) < 0.2] = -1.0
    cl = dict(sigma=sigma, mass1=np.ones(n))
    ks = rng.uniform(0.2, 1.5, (nd, nf))
    taus = list(rng.uniform(0.05, 0.3, nd))
    acc = np.zeros((n, 2 + 3 * nd))
    acc[:, 0] = n_rows
    acc[:, 1] = rng.uniform(0.1, 1.0, n) * n_rows
    d = rng.normal(0, 0.05, (n, nd))
    acc[:, 2::3] = acc[:, 1:2] * d
    acc[:, 3::3] = acc[:, 1:2] * (d ** 2 + rng.uniform(0, 0.01, (n, nd)))
    acc[:, 4::3] = acc[:, 1:2] * rng.normal(1.0, 2.0, (n, nd))
    return cl, ks, taus, acc


def test_offset_table(host):
    from base_amd import hostlib
    cl, ks, taus, acc = example(40, 5, 3, 12)
    acc[4, 1:] = 0.0                                     # counted, no membership weight (acc1 == 0): every derived value 0
    acc[9] = 0.0                                         # never counted
    cl["sigma"][11] = -1.0                               # no filter at all: C = 0, the prior alone
    acc[11, 2:] = 0.0
    got, want = hostlib.offset_table(acc, cl["sigma"], ks, taus), of.star_table(acc, cl, ks, taus)
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-300)
    assert got[4, 0] == 12 and np.all(got[4, 1:] == 0) and np.all(got[9] == 0)
    np.testing.assert_allclose(got[11, 3::4], taus, rtol=1e-15)
    assert np.all(got[11, 2::4] == 0) and np.all(got[11, 4::4] == 0)
    assert got[0, 4] == got[0, 2] / got[0, 3]            # z = mean / sd
    one = hostlib.offset_table(acc[:, :5], cl["sigma"], ks[:1], taus[0])                 # a scalar tau serves every direction
    assert np.array_equal(one, got[:, :6])


def test_offset_dist_table(host):
    from base_amd import hostlib
    rng = np.random.default_rng(7)
    nd, n_rows = 3, 37
    ro = np.zeros((n_rows, 1 + 4 * nd))
    ro[:, 0] = 100
    for j in range(nd):
        N = rng.uniform(50, 90, n_rows)
        ro[:, 1 + 4 * j], ro[:, 2 + 4 * j], ro[:, 3 + 4 * j] = N, N * rng.normal(0, 0.05, n_rows), N * rng.gamma(2, 0.01, n_rows)
        ro[:, 4 + 4 * j] = N * rng.normal(-0.5, 0.3, n_rows)
    ro[3] = 0.0                                          # a row outside the grid stays out of the statistics
    ro[:, 1 + 4 * 1:5 + 4 * 1] = 0.0                     # a direction that touches no star: N = 0 in every row
    got, want = hostlib.offset_dist_table(ro, nd), of.dist_table(ro, nd)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-300)
    assert got[0, 0] == n_rows - 1 and np.all(got[1] == 0)
    assert np.all(got[[0, 2], 13] <= got[[0, 2], 14]) and np.all(got[[0, 2], 14] <= got[[0, 2], 15])
    one = hostlib.offset_dist_table(ro[:1], nd)          # a single-row chain: no spread
    assert np.all(one[[0, 2], 12] == 0) and np.array_equal(one[:, 13], one[:, 15])


def test_files_round_trip(host, tmp_path):
    from base_amd import hostlib
    cl, ks, taus, acc = example(9, 3, 2, 5)
    acc[4, 1:] = 0.0
    tab = hostlib.offset_table(acc, cl["sigma"], ks, taus)
    ids = [f"s{5 * i % 9:02d}" for i in range(9)]
    names = ["absorption", "filter:V"]
    path = str(tmp_path / "x.starOffsets")
    hostlib.write_star_offsets(path, ids, names, tab)
    got_ids, cols, got = hostlib.read_star_offsets(path)
    assert got_ids == ids and cols == ["rows", "member"] + [f"{d}_{c}" for d in names for c in hostlib.OFFSET_STAR_COLUMNS]
    assert hostlib.OFFSET_STAR_COLUMNS == of.STAR_COLUMNS
    assert np.array_equal(got, tab)                      # 17 significant digits: the bits come back
    dt = hostlib.offset_dist_table(np.random.default_rng(1).uniform(0.5, 2.0, (6, 9)), 2)
    path = str(tmp_path / "x.offsetDist")
    hostlib.write_offset_dist(path, names, dt)
    got_names, cols, got = hostlib.read_offset_dist(path)
    assert got_names == names and cols == list(hostlib.OFFSET_DIST_COLUMNS) == list(of.DIST_COLUMNS)
    assert np.array_equal(got, dt)


def test_named_directions(host):
    from base_amd import hostlib
    pack_d = fixture("dsed5")[0]
    filters = [f"F{f}" for f in range(5)]
    ac = np.asarray(pack_d["abs_coeff"], dtype=np.float64)[:5]
    assert np.array_equal(hostlib.offset_direction("absorption", filters, ac), of.direction(pack_d, "absorption"))
    assert np.array_equal(hostlib.offset_direction("distance", filters), of.direction(pack_d, "distance"))
    assert np.array_equal(hostlib.offset_direction("filter:F3", filters), of.direction(pack_d, "filter:3"))
    vals = [1.25, 0.5, -0.125, 0.0, 3.0]
    assert np.array_equal(hostlib.offset_direction(vals, filters), vals)
    assert np.array_equal(hostlib.offset_direction("1.25,0.5,-0.125,0,3", filters), vals)
    assert hostlib.offset_directions(["absorption", "distance", vals], filters, ac).shape == (3, 5)
    for bad in ("filter:nope", "dust", "1,2,3", "1,2,3,4,x"):
        with pytest.raises(hostlib.HostError):
            hostlib.offset_direction(bad, filters, ac)
    with pytest.raises(hostlib.HostError):
        hostlib.offset_direction("absorption", filters)              # no coefficients given


def test_flags_and_yaml_parse(host, tmp_path):
    from base_amd import hostlib
    base = dict(margIsoIncrem=4, nMassRatios=4, nPops=1)
    assert hostlib.star_offsets_settings([]) == dict(base, direction=["absorption", "distance"], tau=[0.1, 0.1])
    d = hostlib.star_offsets_settings(["--direction", "filter:V", "--direction=distance", "--direction", "1,0.5", "--tau", "0.2", "--nPops", "2"])
    assert d == dict(base, nPops=2, direction=["filter:V", "distance", "1,0.5"], tau=[0.2, 0.2, 0.2])
    d = hostlib.star_offsets_settings(["--direction", "absorption", "--tau", "0.05", "--direction", "distance", "--tau", "0.3", "--margIsoIncrem", "2"])
    assert d == dict(base, margIsoIncrem=2, direction=["absorption", "distance"], tau=[0.05, 0.3])
    y = tmp_path / "so.yaml"
    y.write_text("sampleMass:\n  margIsoIncrem: 6\n  nMassRatios: 5\nfilterCheck:\n  nPops: 2\nstarOffsets:\n  nMassRatios: 7\n"
                 "  direction: distance filter:B\n  tau: 0.2 0.4\n")
    d = hostlib.star_offsets_settings(["--config", str(y)])          # sampleMass's grid is the default; other programs' keys are not read
    assert d == dict(margIsoIncrem=6, nMassRatios=7, nPops=1, direction=["distance", "filter:B"], tau=[0.2, 0.4])
    d = hostlib.star_offsets_settings(["--config", str(y), "--direction", "absorption", "--tau", "0.1"])      # a flag replaces the file's list
    assert d["direction"] == ["absorption"] and d["tau"] == [0.1]
    for bad in (["--nPops", "3"], ["--tau", "0"], ["--tau", "-1"], ["--tau", "0.1", "--tau", "0.2", "--tau", "0.3"], ["--tau", "x"],
                ["--direction", "a", "--direction", "b", "--direction", "c", "--direction", "d", "--direction", "e"]):
        with pytest.raises(hostlib.HostError):
            hostlib.star_offsets_settings(bad)
