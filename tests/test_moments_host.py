"""CPU tests of the starSummary host side: b9h_star_table against the formulas, the .starSummary file, the numpy
reference's own sanity (tests/moments_ref.py), and the statistical checks of tests/test_gpu_moments.py run on numpy draws
from the reference weights -- each must pass on the reference and reject a mutated one."""
import numpy as np
import pytest

import moments_ref as mr
from base_amd import abi, hostlib, synth
from conftest import build_problem


@pytest.fixture(scope="module")
def host():
    from base_amd import host_build
    host_build.build_host()
    return hostlib.load()


def example_acc():
    rng = np.random.default_rng(5)
    n = 12
    rows = rng.integers(1, 50, n).astype(float)
    member = rows * rng.uniform(0.01, 1.0, n)
    mass, sd = rng.uniform(0.2, 4.0, n), rng.uniform(1e-4, 0.3, n)
    q, qsd = rng.uniform(0.0, 0.9, n), rng.uniform(0.0, 0.2, n)
    acc = np.stack([rows, member, member * mass, member * (sd ** 2 + mass ** 2), member * q, member * (qsd ** 2 + q ** 2),
                    member * rng.uniform(0, 1, n), member * rng.uniform(0, 1, n)], axis=1)
    acc[3] = [7.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]                     # counted rows, no membership weight
    acc[4] = 0.0                                                         # a star no row contributed to
    m = 1.2345678901234567                                               # a one-node posterior: the variance comes out slightly negative
    acc[5] = [3.0, 2.5, 2.5 * m, 2.5 * m * m * (1 - 2 ** -50), 0.0, 0.0, 0.0, 0.0]
    return acc, mass, sd


def test_star_table_matches_formulas(host):
    acc, mass, sd = example_acc()
    t = hostlib.star_table(acc)
    np.testing.assert_array_equal(t[:, 0], acc[:, 0])
    np.testing.assert_allclose(t, mr.table(acc), rtol=1e-15, atol=0)
    ok = np.ones(len(acc), bool); ok[[3, 4, 5]] = False
    np.testing.assert_allclose(t[ok, 2], mass[ok], rtol=1e-14)
    np.testing.assert_allclose(t[ok, 3], sd[ok], rtol=1e-6)
    np.testing.assert_allclose(t[ok, 1], acc[ok, 1] / acc[ok, 0], rtol=1e-15)
    np.testing.assert_allclose(t[ok, 6], acc[ok, 6] / acc[ok, 1], rtol=1e-15)
    np.testing.assert_allclose(t[ok, 7], acc[ok, 7] / acc[ok, 1], rtol=1e-15)
    assert np.array_equal(t[3], [7, 0, 0, 0, 0, 0, 0, 0]) and np.all(t[4] == 0)      # acc1 == 0: every derived value is 0
    assert acc[5, 3] / acc[5, 1] - (acc[5, 2] / acc[5, 1]) ** 2 < 0           # the raw variance IS negative ...
    assert t[5, 3] == 0.0 and t[5, 2] == pytest.approx(1.2345678901234567, rel=1e-15)   # ... and clamps to 0
    one = acc.copy(); one[:, 7] = 0.0                                      # one population: pPop2 is 0
    assert np.all(hostlib.star_table(one)[:, 7] == 0)


@pytest.mark.parametrize("n_pops", [1, 2])
def test_star_summary_round_trip(host, tmp_path, n_pops):
    acc, _, _ = example_acc()
    ids = [f"s{7 * i % 12:03d}" for i in range(len(acc))]                   # not sorted: the file keeps the caller's order
    path = str(tmp_path / "x.starSummary")
    hostlib.write_star_summary(path, ids, acc, n_pops)
    lines = open(path).read().splitlines()
    want_cols = ["rows", "member", "mass", "massSd", "massRatio", "massRatioSd", "pBinary"] + (["pPop2"] if n_pops == 2 else [])
    assert lines[0].split() == ["id"] + want_cols and len(lines) == 1 + len(acc)
    assert all(len(l.split()) == 1 + len(want_cols) for l in lines[1:])
    got_ids, cols, tab = hostlib.read_star_summary(path)
    assert got_ids == ids and cols == want_cols
    np.testing.assert_allclose(tab, hostlib.star_table(acc)[:, :len(want_cols)], rtol=0, atol=0.5e-6)
    assert np.array_equal(tab[:, 0], acc[:, 0])


# ---- the reference's own sanity -------------------------------------------------------------------------------------------
def case1():
    pack_d, cl, pack, stars, priors, _ = build_problem("dsed", 5, n_stars=130, wd_frac=0.1, n_y=3, n_pops=2, seed=12)
    rows = synth.walker_params(cl["truth"], 3, seed=3, scale=0.3)
    rows[:, abi.P_LAMBDA] = np.clip(rows[:, abi.P_LAMBDA], 0.05, 0.95)
    return pack_d, cl, rows


@pytest.fixture(scope="module")
def case1_nodes():
    pack_d, cl, rows = case1()
    return pack_d, cl, rows, mr.star_nodes(pack_d, cl, rows[0], 2, 2, 2)


def test_reference_sanity(case1_nodes):
    pack_d, cl, rows, nodes = case1_nodes
    for nd in nodes:
        if len(nd[0]):
            assert mr.weights(nd)[0].sum() == pytest.approx(1.0, abs=1e-12)
    x = mr.increments(pack_d, cl, rows[0], 2, 2, 2)
    assert np.all(x[:, mr.BINARY] <= x[:, mr.MEMBER] * (1 + 1e-12)) and np.all(x[:, mr.POP1] <= x[:, mr.MEMBER] * (1 + 1e-12))
    assert np.all((x[:, mr.MEMBER] >= 0) & (x[:, mr.MEMBER] <= 1)) and (x[:, mr.ROWS] == 1).sum() > 100
    # one mass ratio: no companion anywhere
    x1 = mr.increments(pack_d, cl, rows[0], 2, 2, 1)
    assert np.all(x1[:, [mr.Q, mr.QSQ, mr.BINARY]] == 0) and np.any(x1[:, mr.M1] > 0)
    # a row outside the grid contributes nothing
    out = rows[0].copy(); out[abi.P_LOGAGE] = pack_d["log_age"][-1] + 1.0
    assert np.all(mr.increments(pack_d, cl, out, 2, 2, 2) == 0)
    # two populations at lambda -> 1 reproduce one population
    # (at the limit itself: log(1 - lambda) = -inf takes every node of the second population out; short of it a star whose
    #  second-population likelihood is e^20 times the first's still feels a weight of 1e-15)
    near = rows[0].copy(); near[abi.P_LAMBDA] = 1.0
    a, b = mr.increments(pack_d, cl, near, 2, 2, 2), mr.increments(pack_d, cl, rows[0], 1, 2, 2)
    np.testing.assert_allclose(a[:, :7], b[:, :7], rtol=1e-12, atol=0)
    assert np.all(a[:, mr.POP1] == 0)


def test_statistical_checks_pass_on_the_reference_and_reject_mutations(case1_nodes):
    """The two checks of test_gpu_moments.py::test_statistics_against_device_draws, on 1000 numpy draws per star from the
    reference weights.  Both pass on the reference's own table.  The binomial check rejects the reference with the
    population weight left out (and cannot see the second moments, which it does not read); the mean-mass check rejects
    the reference whose second moments are built from M1 instead of M1^2 (every star heavier than 1 Msun loses its
    spread) -- each check rejects a mutation, each mutation is rejected by a check."""
    pack_d, cl, rows, _ = case1_nodes
    R = 1000

    def run(row, **mutation):
        nodes = mr.star_nodes(pack_d, cl, row, 2, 2, 2)
        mean_m, n_bin, n_p1 = mr.numpy_draws(nodes, R, seed=11)
        ref_mo = [mr.skewness(nd) if len(nd[0]) else None for nd in nodes]
        acc = mr.accumulate(pack_d, cl, row, 2, 2, 2, **mutation)
        tab = mr.table(acc)
        return mr.binomial_pvalues(tab, acc, n_bin, n_p1, R, 2), mr.mass_z(tab, mean_m, ref_mo, R)

    # the case's rows carry lambda = 0.5, where leaving the population weight out changes nothing: the mutations are judged
    # at lambda = 0.3 as well as the reference itself
    skew = rows[0].copy(); skew[abi.P_LAMBDA] = 0.3
    for row in (rows[0], skew):
        p, z = run(row)
        print(f"reference, lambda {row[abi.P_LAMBDA]}: {len(p)} binomial tests, smallest p {p.min():.3g}; {len(z)} guarded stars, largest |z| {np.abs(z).max():.3g}")
        assert len(p) >= 150 and p.min() >= mr.P_MIN
        assert len(z) >= 60 and np.abs(z).max() <= mr.Z_MAX
    p_a, z_a = run(skew, second_moment_power=1)
    print(f"second moments from M1: largest |z| {np.abs(z_a).max():.3g}, smallest p {p_a.min():.3g}")
    assert not np.abs(z_a).max() <= mr.Z_MAX
    p_b, z_b = run(skew, drop_pop_weight=True)
    print(f"population weight left out: smallest p {p_b.min():.3g}, largest |z| {np.abs(z_b).max():.3g}")
    assert p_b.min() < mr.P_MIN
