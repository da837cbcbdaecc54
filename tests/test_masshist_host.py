"""CPU tests of the massFunction host side and of the checkers themselves: the comparators of tests/masshist_check.py must
accept the reference (tests/masshist_ref.py) and reject five mutated references; b9h_mass_function_table against the numpy
restatement; the two files; massFunction's flags and YAML keys."""
import numpy as np
import pytest

import masshist_check as hc
import masshist_ref as hr
from base_amd import abi, hostlib, synth
from conftest import build_problem


@pytest.fixture(scope="module")
def host():
    from base_amd import host_build
    host_build.build_host()
    return hostlib.load()


# ---- the checker's own power ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case1():
    pack_d, cl, pack, stars, priors, _ = build_problem("dsed", 5, n_stars=130, wd_frac=0.1, n_y=3, n_pops=2, seed=12)
    rows = synth.walker_params(cl["truth"], 3, seed=3, scale=0.3)
    rows[:, abi.P_LAMBDA] = 0.3                          # (at 0.5 leaving the population weight out changes nothing)
    nodes = hr.nodes_of_rows(pack_d, cl, rows, 2, 2, 2)
    return pack_d, cl, rows, nodes


def reference(case1, quantity, edges, **mutation):
    pack_d, cl, rows, nodes = case1
    x = hr.all_increments(pack_d, cl, rows, 2, 2, 2, quantity, edges, nodes_by_row=nodes, **mutation)
    return hr.accumulate(x), hr.row_sums(x)


def rejects(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


MUTATIONS = [
    ("bins closed on the right", hr.PRIMARY, dict(right_closed=True)),
    ("membership weight dropped", hr.PRIMARY, dict(drop_membership=True)),
    ("SECONDARY binned on q instead of q M1", hr.SECONDARY, dict(secondary_on_q=True)),
    ("population weight dropped", hr.PRIMARY, dict(drop_pop_weight=True)),
    ("normalised by the bin range instead of all nodes", hr.PRIMARY, dict(normalise_in_range=True)),
]


@pytest.mark.parametrize("what,quantity,mutation", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_comparators_reject_mutated_references(case1, what, quantity, mutation):
    pack_d, cl, rows, nodes = case1
    n_nodes, n_stars = 712, len(cl["mass1"])
    edges = hc.quantile_edges(nodes, quantity, 24)
    if "right_closed" in mutation:
        # closing the bins on the right moves a node only when it sits ON an edge: put every other edge on a node value
        v, _ = hc.reference_values(nodes, quantity)
        v = np.unique(v)
        edges = edges.copy()
        for b in range(2, 23, 2):
            edges[b] = v[np.searchsorted(v, edges[b])]
        assert np.all(np.diff(edges) > 0)
    if "normalise_in_range" in mutation:
        edges = edges[6:19]                              # a range that misses part of the grid
    want_star, want_rows = reference(case1, quantity, edges)
    # the reference passes its own comparators, and so does a copy perturbed at a tenth of the tolerance
    hc.assert_hist(want_star, want_rows, want_star, want_rows, n_nodes, n_stars)
    hc.assert_hist(want_star * (1 + 1e-10), want_rows * (1 - 1e-10), want_star, want_rows, n_nodes, n_stars)
    got_star, got_rows = reference(case1, quantity, edges, **mutation)
    print(f"{what}: largest relative difference star_hist {hc.largest_rel(got_star, want_star, 0):.3g}, row_hist {hc.largest_rel(got_rows, want_rows, 0):.3g}")
    assert rejects(hc.assert_star_hist, got_star, want_star, n_nodes, len(rows))
    assert rejects(hc.assert_row_hist, got_rows, want_rows, n_nodes, n_stars)


def test_reference_sanity(case1):
    pack_d, cl, rows, nodes = case1
    for quantity in (hr.PRIMARY, hr.SECONDARY, hr.SYSTEM):
        edges = hc.quantile_edges(nodes, quantity, 24)
        star, rws = reference(case1, quantity, edges)
        nb = 24
        assert np.all(star[:, :nb].sum(axis=1) <= star[:, nb] * (1 + 1e-12))
        if quantity != hr.SECONDARY:                     # the edges span every node: the bins hold everything
            np.testing.assert_allclose(star[:, :nb].sum(axis=1), star[:, nb], rtol=1e-12)
        np.testing.assert_allclose(rws.sum(axis=0), star.sum(axis=0), rtol=1e-12)
        # disjoint edge sets compose exactly: the normalisation ignores the edges
        a, _ = reference(case1, quantity, edges[:13])
        b, _ = reference(case1, quantity, edges[12:])
        assert np.array_equal(a[:, :12], star[:, :12]) and np.array_equal(b[:, :12], star[:, 12:24])
    live, two, inside = hc.non_vacuity(reference(case1, hr.PRIMARY, hc.quantile_edges(nodes, hr.PRIMARY, 64))[0], 3)
    assert two >= live // 2 and live >= 100
    out = rows[0].copy(); out[abi.P_LOGAGE] = pack_d["log_age"][-1] + 1.0
    assert np.all(hr.increments(pack_d, cl, out, 2, 2, 2, hr.PRIMARY, edges) == 0)


# ---- the host table -----------------------------------------------------------------------------------------------------------
def example_rows(n_rows, n_bins, seed=4):
    rng = np.random.default_rng(seed)
    rh = rng.gamma(2.0, 3.0, (n_rows, n_bins + 1))
    rh[:, n_bins] = rh[:, :n_bins].sum(axis=1) * 1.1
    return rh


@pytest.mark.parametrize("n_rows,n_bins", [(37, 24), (1, 5), (2, 1), (100, 64)])
def test_mass_function_table(host, n_rows, n_bins):
    edges = 0.1 * 80.0 ** (np.arange(n_bins + 1) / n_bins)
    rh = example_rows(n_rows, n_bins)
    if n_rows > 2:
        rh[3] = 0.0                                      # a row with no members (outside the grid) stays out of the statistics
    got, want = hostlib.mass_function_table(rh, edges), hr.table(rh, edges)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-300)
    assert np.array_equal(got[:, 0], edges[:-1]) and np.array_equal(got[:, 1], edges[1:])
    if n_rows > 2:
        kept = np.delete(rh, 3, axis=0)
        np.testing.assert_allclose(got[:, 2], kept[:, :n_bins].mean(axis=0), rtol=1e-12)
        assert np.all(got[:, 4] <= got[:, 5]) and np.all(got[:, 5] <= got[:, 6])
    if n_rows == 1:                                      # a single-row chain: no spread, every percentile is the row
        assert np.all(got[:, 3] == 0) and np.array_equal(got[:, 4], rh[0, :n_bins]) and np.array_equal(got[:, 6], rh[0, :n_bins])


def test_mass_function_table_without_members_and_linear_bins(host):
    edges = np.linspace(0.0, 8.0, 9)                     # lo = 0: no logarithmic width, dNdlogM is 0 there
    rh = np.zeros((5, 9))
    got = hostlib.mass_function_table(rh, edges)
    assert np.all(got[:, 2:] == 0) and np.array_equal(got[:, 0], edges[:-1])
    rh = example_rows(6, 8)
    got = hostlib.mass_function_table(rh, edges)
    assert got[0, 7] == 0 and np.all(got[1:, 7] > 0)
    np.testing.assert_allclose(got, hr.table(rh, edges), rtol=1e-12, atol=1e-300)


def test_files_round_trip(host, tmp_path):
    n_bins = 7
    edges = 0.1 * 80.0 ** (np.arange(n_bins + 1) / n_bins)
    tab = hostlib.mass_function_table(example_rows(20, n_bins), edges)
    path = str(tmp_path / "x.massFunction")
    hostlib.write_mass_function(path, tab)
    _, cols, got = hostlib.read_table_file(path, None)
    assert cols == list(hostlib.MASS_FUNCTION_COLUMNS) and got.shape == (n_bins, 8)
    np.testing.assert_allclose(got, tab, rtol=0, atol=0.5e-6)
    rng = np.random.default_rng(2)
    sh = rng.uniform(0, 1, (9, n_bins + 1))
    sh[:, n_bins] = sh[:, :n_bins].sum(axis=1) + 0.5
    sh[4] = 0.0                                          # no membership weight: zeros
    ids = [f"s{5 * i % 9:02d}" for i in range(9)]
    path = str(tmp_path / "x.starMassHist")
    hostlib.write_star_mass_hist(path, ids, sh, 12)
    got_ids, cols, got = hostlib.read_table_file(path, "id")
    assert got_ids == ids and cols == ["rows", "member"] + [f"bin{b}" for b in range(n_bins)]
    assert np.all(got[:, 0] == 12) and np.all(got[4, 1:] == 0)
    live = np.arange(9) != 4
    np.testing.assert_allclose(got[:, 1], sh[:, n_bins] / 12, rtol=0, atol=0.5e-6)
    np.testing.assert_allclose(got[live, 2:], sh[live, :n_bins] / sh[live, n_bins:], rtol=0, atol=0.5e-6)


# ---- flags and YAML -----------------------------------------------------------------------------------------------------------
def test_flags_and_yaml_parse(host, tmp_path):
    d, edges = hostlib.mass_function_settings([], m_wd_up=8.0)
    assert d == dict(nBins=24, minMass=0.1, maxMass=8.0, linearBins=0, quantity=abi.HQ_PRIMARY, perStar=0, margIsoIncrem=4, nMassRatios=4, nPops=1)
    assert len(edges) == 25 and edges[0] == 0.1 and edges[-1] == 8.0 and np.all(np.diff(edges) > 0)
    np.testing.assert_allclose(edges, 0.1 * 80.0 ** (np.arange(25) / 24), rtol=1e-14)
    d, edges = hostlib.mass_function_settings(["--nBins", "10", "--minMass", "0.5", "--maxMass=5.5", "--linearBins", "--quantity", "system", "--perStar",
                                               "--margIsoIncrem", "2", "--nMassRatios", "3"])
    assert d == dict(nBins=10, minMass=0.5, maxMass=5.5, linearBins=1, quantity=abi.HQ_SYSTEM, perStar=1, margIsoIncrem=2, nMassRatios=3, nPops=1)
    np.testing.assert_allclose(edges, np.linspace(0.5, 5.5, 11), rtol=1e-14)
    y = tmp_path / "mf.yaml"
    y.write_text("simCluster:\n  minMass: 0.4\nmassFunction:\n  nBins: 64\n  minMass: 0.2\n  maxMass: 6.0\n  linearBins: 0\n  quantity: secondary\n"
                 "  margIsoIncrem: 3\n  nMassRatios: 5\n  nPops: 2\n")
    d, edges = hostlib.mass_function_settings(["--config", str(y)])
    assert d == dict(nBins=64, minMass=0.2, maxMass=6.0, linearBins=0, quantity=abi.HQ_SECONDARY, perStar=0, margIsoIncrem=3, nMassRatios=5, nPops=2)
    assert len(edges) == 65
    d, _ = hostlib.mass_function_settings(["--config", str(y), "--nBins", "8", "--minMass", "0.3"])       # a flag overrides the file
    assert d["nBins"] == 8 and d["minMass"] == 0.3
    for bad in (["--nBins", "0"], ["--nBins", "65"], ["--quantity", "total"], ["--minMass", "9"], ["--minMass", "0"]):
        with pytest.raises(hostlib.HostError):
            hostlib.mass_function_settings(bad)


def test_short_and_long_flags(host):
    """--minMass / --maxMass are massFunction's own spellings of --massFunctionMinMass / --massFunctionMaxMass: both give the same
    settings, on this program's command line only -- the shared table gives the short names to simCluster --, and massFunction
    takes no other program's short flag for a key of its own."""
    from cli_util import settings_dump
    short = hostlib.mass_function_settings(["--minMass", "0.5", "--maxMass=5.5"])
    long_ = hostlib.mass_function_settings(["--massFunctionMinMass", "0.5", "--massFunctionMaxMass=5.5"])
    assert short[0] == long_[0] and short[0]["minMass"] == 0.5 and short[0]["maxMass"] == 5.5 and np.array_equal(short[1], long_[1])
    assert settings_dump(["--minMass", "0.5", "--maxMass=5.5"]) == {"simCluster.minMass": "0.5", "simCluster.maxMass": "5.5"}
    assert settings_dump(["--massFunctionMinMass", "0.5"]) == {"massFunction.minMass": "0.5"}
    # --nPops stays simCluster's here: massFunction's population count comes from the YAML only
    assert hostlib.mass_function_settings(["--nPops", "2"])[0] == hostlib.mass_function_settings([])[0]
    assert hostlib.mass_function_settings(["--perStar=0"])[0]["perStar"] == 0 and hostlib.mass_function_settings(["--perStar"])[0]["perStar"] == 1
    with pytest.raises(hostlib.HostError, match="unexpected argument '0'"):
        hostlib.mass_function_settings(["--perStar", "0"])
    with pytest.raises(hostlib.HostError):
        hostlib.mass_function_settings(["--perRow"])                    # modelScore's
