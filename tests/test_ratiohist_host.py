"""CPU tests of the binaryStats host side and of the checkers themselves: the marginals of the reference
(tests/ratiohist_ref.py) against masshist_ref and moments_ref; the comparators the GPU suite uses (tests/masshist_check.py, the
tolerance of b9_mass_hist) must accept the reference and reject its five mutations; b9h_binary_table, b9h_ratio_dist_table and
b9h_star_ratio_table against the numpy restatement; the three files; the argument errors."""
import numpy as np
import pytest

import masshist_check as hc
import masshist_ref as hr
import moments_ref as mr
import ratiohist_ref as rr
from base_amd import abi, hostlib, synth
from conftest import build_problem

K, Q, N_NODES = 1, 4, 356                                 # parsec, 8 filters: 89 EEP intervals x K x Q


@pytest.fixture(scope="module")
def host():
    from base_amd import host_build
    host_build.build_host()
    return hostlib.load()


@pytest.fixture(scope="module")
def case1():
    pack_d, cl, pack, stars, priors, _ = build_problem("parsec", 8, n_stars=130, wd_frac=0.1, seed=12)
    rows = synth.walker_params(cl["truth"], 3, seed=3, scale=0.3)
    nodes = hr.nodes_of_rows(pack_d, cl, rows, 1, K, Q)
    return pack_d, cl, rows, nodes


def rejects(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


# ---- the reference's marginals ----------------------------------------------------------------------------------------------
def test_reference_marginals(case1):
    pack_d, cl, rows, nodes = case1
    n_mbins = 6
    edges = hc.quantile_edges(nodes, hr.PRIMARY, n_mbins)
    star, rws = rr.reference(pack_d, cl, rows, 1, K, Q, edges, nodes)
    assert star.shape == (130, n_mbins * Q + 1) and rws.shape == (3, n_mbins * Q + 1)
    # sum_j = the primary-mass histogram
    x = hr.all_increments(pack_d, cl, rows, 1, K, Q, hr.PRIMARY, edges, nodes_by_row=nodes)
    want_star, want_rows = hr.accumulate(x), hr.row_sums(x)
    np.testing.assert_allclose(star[:, :-1].reshape(130, n_mbins, Q).sum(axis=2), want_star[:, :-1], rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(rws[:, :-1].reshape(3, n_mbins, Q).sum(axis=2), want_rows[:, :-1], rtol=1e-12, atol=1e-300)
    assert np.array_equal(star[:, -1], want_star[:, -1])
    # one enclosing bin: sum_{j >= 1} = BINARY, sum j / Q cell = the Q sum
    one, _ = rr.reference(pack_d, cl, rows, 1, K, Q, [0.0, np.finfo(float).max], nodes)
    mom = sum(mr.increments(pack_d, cl, par, 1, K, Q, nodes=nodes[r]) for r, par in enumerate(rows))
    np.testing.assert_allclose(one[:, 1:Q].sum(axis=1), mom[:, mr.BINARY], rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose((one[:, :Q] * (np.arange(Q) / Q)).sum(axis=1), mom[:, mr.Q], rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(one[:, Q], mom[:, mr.MEMBER], rtol=1e-12, atol=1e-300)
    # a cell does not depend on the other bins; a row outside the grid adds nothing
    part, _ = rr.reference(pack_d, cl, rows, 1, K, Q, edges[2:5], nodes)
    assert np.array_equal(part[:, :2 * Q], star[:, 2 * Q:4 * Q])
    out = rows[0].copy(); out[abi.P_LOGAGE] = pack_d["log_age"][-1] + 1.0
    assert np.all(rr.increments(pack_d, cl, out, 1, K, Q, edges) == 0)
    # the case is not vacuous: mass bins, companion ratios, WD-stage stars
    cells = star[:, :-1].reshape(130, n_mbins, Q)
    assert (cells.sum(axis=(0, 2)) > 1e-3).sum() >= 2 and (cells.sum(axis=(0, 1))[1:] > 1e-3).sum() >= 2
    wd = np.asarray(cl["stage"]) == abi.STAGE_WD
    assert wd.any() and cells[wd, :, 0].sum() > 1e-3 and np.all(cells[wd, :, 1:] == 0)


# ---- the checker's own power ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutation", rr.MUTATIONS)
def test_comparators_reject_mutated_references(case1, mutation):
    pack_d, cl, rows, nodes = case1
    n_stars = len(cl["mass1"])
    edges = hc.quantile_edges(nodes, hr.PRIMARY, 6)
    if mutation == "normalise_in_range":
        edges = edges[2:5]                               # a range that misses part of the grid
    want_star, want_rows = rr.reference(pack_d, cl, rows, 1, K, Q, edges, nodes)
    hc.assert_hist(want_star, want_rows, want_star, want_rows, N_NODES, n_stars)
    hc.assert_hist(want_star * (1 + 1e-10), want_rows * (1 - 1e-10), want_star, want_rows, N_NODES, n_stars)
    got_star, got_rows = rr.reference(pack_d, cl, rows, 1, K, Q, edges, nodes, **{mutation: True})
    print(f"{mutation}: largest relative difference star_cells {hc.largest_rel(got_star, want_star, 0):.3g}, row_cells {hc.largest_rel(got_rows, want_rows, 0):.3g}")
    assert rejects(hc.assert_star_hist, got_star, want_star, N_NODES, len(rows))
    assert rejects(hc.assert_row_hist, got_rows, want_rows, N_NODES, n_stars)


# ---- the host tables ------------------------------------------------------------------------------------------------------------
def example_cells(n_rows, n_mbins, q, seed=4):
    rng = np.random.default_rng(seed)
    rc = rng.gamma(2.0, 3.0, (n_rows, n_mbins * q + 1))
    rc[:, -1] = rc[:, :-1].sum(axis=1) * 1.1
    return rc


@pytest.mark.parametrize("n_rows,n_mbins,q,q_min", [(37, 4, 4, 0.0), (37, 4, 4, 0.5), (37, 4, 4, 0.51), (1, 3, 5, 0.2), (2, 1, 1, 0.0), (60, 16, 8, 0.75),
                                                    (11, 2, 3, 1.0)])
def test_tables_against_numpy(host, n_rows, n_mbins, q, q_min):
    edges = 0.1 * 80.0 ** (np.arange(n_mbins + 1) / n_mbins)
    rc = example_cells(n_rows, n_mbins, q)
    if n_rows > 10:
        rc[3] = 0.0                                      # a row with no members stays out of every line
        rc[5, q:2 * q] = 0.0                             # N_b = 0 for mass bin 1 in rows 5 and 6: out of that line only
        rc[6, q:2 * q] = 0.0
    got = hostlib.binary_table(rc, edges, q, q_min)
    np.testing.assert_allclose(got, rr.binary_table(rc, edges, q, q_min), rtol=1e-12, atol=1e-300)
    assert np.array_equal(got[:-1, 0], edges[:-1]) and np.array_equal(got[:-1, 1], edges[1:]) and got[-1, 0] == edges[0] and got[-1, 1] == edges[-1]
    if n_rows > 10:
        assert np.all(got[[0, 2, n_mbins], 2] == n_rows - 1) and got[1, 2] == n_rows - 3
    assert np.all(got[:, 8] >= 0) and np.all(got[:, 8] <= 1) and np.all(got[:, 10] <= got[:, 11]) and np.all(got[:, 11] <= got[:, 12])
    dist = hostlib.ratio_dist_table(rc, n_mbins, q)
    np.testing.assert_allclose(dist, rr.ratio_dist_table(rc, n_mbins, q), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(dist[:, :, 3].sum(axis=1), 1.0, rtol=1e-12)          # a line's mean fractions sum to 1
    sc = example_cells(9, n_mbins, q, seed=7)
    sc[:, -1] *= 40.0
    sc[4] = 0.0                                          # no membership weight: zeros
    per = hostlib.star_ratio_table(sc, n_mbins, q, 50, q_min)
    np.testing.assert_allclose(per, rr.star_ratio_table(sc, n_mbins, q, 50, q_min), rtol=1e-12, atol=1e-300)
    assert np.all(per[:, 0] == 50) and np.all(per[4, 1:] == 0)
    np.testing.assert_allclose(per[:, 4:].sum(axis=1), per[:, 2], rtol=1e-12)


def test_q_min_on_a_node_counts_it(host):
    """q_min = j / Q exactly counts node j; the next double above it does not."""
    q, n_mbins = 4, 2
    rc = example_cells(20, n_mbins, q)
    edges = np.array([0.1, 1.0, 8.0])
    at = hostlib.binary_table(rc, edges, q, 0.5)
    above = hostlib.binary_table(rc, edges, q, np.nextafter(0.5, 1.0))
    cells = rc[:, :-1].reshape(20, n_mbins, q)
    N = cells.sum(axis=2)
    np.testing.assert_allclose(at[:n_mbins, 8], (cells[:, :, 2:].sum(axis=2) / N).mean(axis=0), rtol=1e-12)
    np.testing.assert_allclose(above[:n_mbins, 8], (cells[:, :, 3:].sum(axis=2) / N).mean(axis=0), rtol=1e-12)
    zero = hostlib.binary_table(rc, edges, q, 0.0)      # the default: every j >= 1, never j = 0
    np.testing.assert_allclose(zero[:n_mbins, 8], (cells[:, :, 1:].sum(axis=2) / N).mean(axis=0), rtol=1e-12)
    per_at, per_above = hostlib.star_ratio_table(rc, n_mbins, q, 20, 0.5), hostlib.star_ratio_table(rc, n_mbins, q, 20, np.nextafter(0.5, 1.0))
    np.testing.assert_allclose(per_at[:, 3], per_at[:, 6] + per_at[:, 7], rtol=1e-12)
    np.testing.assert_allclose(per_above[:, 3], per_above[:, 7], rtol=1e-12)


def test_tables_without_a_usable_row(host):
    edges = np.array([0.1, 1.0, 8.0])
    for rc in (np.zeros((5, 9)), np.zeros((0, 9))):
        got = hostlib.binary_table(rc, edges, 4, 0.0)
        assert np.all(got[:, 2:] == 0) and np.array_equal(got[:, 0], [0.1, 1.0, 0.1]) and np.array_equal(got[:, 1], [1.0, 8.0, 8.0])
        dist = hostlib.ratio_dist_table(rc, 2, 4)
        assert np.all(dist[:, :, 2:] == 0) and np.array_equal(dist[1, :, 0], np.arange(4)) and np.array_equal(dist[2, :, 1], np.arange(4) / 4)
    rc = example_cells(5, 2, 4)
    rc[:, -1] = 0.0                                      # cells without membership: still no usable row
    assert np.all(hostlib.binary_table(rc, edges, 4, 0.0)[:, 2:] == 0)
    per = hostlib.star_ratio_table(np.zeros((3, 9)), 2, 4, 0)
    assert np.all(per == 0)


def test_files_round_trip(host, tmp_path):
    n_mbins, q = 3, 4
    edges = np.array([0.1, 0.5, 1.5, 8.0])
    rc = example_cells(20, n_mbins, q)
    frac, dist = hostlib.binary_table(rc, edges, q, 0.5), hostlib.ratio_dist_table(rc, n_mbins, q)
    path = str(tmp_path / "x.binaryFraction")
    hostlib.write_binary_fraction(path, frac)
    labels, cols, got = hostlib.read_table_file(path, "bin")
    assert labels == ["0", "1", "2", "all"] and cols == list(hostlib.BINARY_FRACTION_COLUMNS) and np.array_equal(got, frac)
    path = str(tmp_path / "x.ratioDist")
    hostlib.write_ratio_dist(path, dist)
    labels, cols, got = hostlib.read_table_file(path, "bin")
    assert labels == [b for b in ("0", "1", "2", "all") for _ in range(q)] and cols == list(hostlib.RATIO_DIST_COLUMNS)
    assert np.array_equal(got, dist.reshape(-1, 8))
    sc = example_cells(9, n_mbins, q, seed=7)
    sc[4] = 0.0
    per = hostlib.star_ratio_table(sc, n_mbins, q, 12, 0.5)
    ids = [f"s{5 * i % 9:02d}" for i in range(9)]
    path = str(tmp_path / "x.starRatio")
    hostlib.write_star_ratio(path, ids, per)
    got_ids, cols, got = hostlib.read_table_file(path, "id")
    assert got_ids == ids and cols == ["rows", "member", "inRange", "pBinaryAbove"] + [f"q{j}" for j in range(q)] and np.array_equal(got, per)


def test_argument_errors(host):
    rc, edges = example_cells(4, 2, 4), np.array([0.1, 1.0, 8.0])
    for bad in (lambda: hostlib.binary_table(rc, edges, 4, -0.1), lambda: hostlib.binary_table(rc, edges, 4, 1.5),
                lambda: hostlib.binary_table(rc, edges, 4, float("nan")), lambda: hostlib.binary_table(np.zeros((4, 1)), edges[:1], 4),
                lambda: hostlib.ratio_dist_table(rc, 0, 4), lambda: hostlib.ratio_dist_table(rc, 2, 0),
                lambda: hostlib.star_ratio_table(rc, 2, 4, 10, 2.0), lambda: hostlib.star_ratio_table(rc, 2, 4, -1)):
        with pytest.raises(hostlib.HostError):
            bad()
    lib = hostlib.load()                                 # the C surface itself: NULL pointers, n_mbins and Q below 1
    import ctypes as C
    dp = C.POINTER(C.c_double)
    out = np.full(3 * 13, 7.25)
    assert lib.b9h_binary_table(None, 4, edges.ctypes.data_as(dp), 2, 4, 0.0, out.ctypes.data_as(dp)) != 0
    assert lib.b9h_binary_table(rc.ctypes.data_as(dp), 4, None, 2, 4, 0.0, out.ctypes.data_as(dp)) != 0
    assert lib.b9h_binary_table(rc.ctypes.data_as(dp), 4, edges.ctypes.data_as(dp), 0, 4, 0.0, out.ctypes.data_as(dp)) != 0
    assert lib.b9h_binary_table(rc.ctypes.data_as(dp), 4, edges.ctypes.data_as(dp), 2, 0, 0.0, out.ctypes.data_as(dp)) != 0
    assert lib.b9h_ratio_dist_table(rc.ctypes.data_as(dp), 4, 2, 4, None) != 0
    assert lib.b9h_star_ratio_table(None, 4, 2, 4, 0.0, 10, out.ctypes.data_as(dp)) != 0
    assert np.all(out == 7.25) and b"b9h_star_ratio_table" in lib.b9h_last_error()


def test_flags_parse(host):
    """--massEdges / --massBins / --qMin reach binaryStats' keys; --nPops is binaryStats' own spelling on its command line only."""
    from cli_util import settings_dump
    assert settings_dump(["--massEdges", "0.1,0.8,2.0", "--qMin", "0.5"]) == {"binaryStats.massEdges": "0.1,0.8,2.0", "binaryStats.qMin": "0.5"}
    assert settings_dump(["--massBins=5", "--binaryStatsNPops", "2"]) == {"binaryStats.massBins": "5", "binaryStats.nPops": "2"}
