"""b9_ratio_hist (the binaryStats counterpart) on the GPU: star_cells and row_cells against the numpy statement
tests/ratiohist_ref.py, the edges of the star, column-tile and node shapes, the mass-bin seam on the device's own bits, the ties
to b9_star_moments and b9_mass_hist, bit-for-bit invariances, the sampler left alone, the errors, every kernel instance, and the
CLI.  Each test makes its own short-lived engine on small packs; a case's reference nodes are computed once and shared.

Tolerance of every comparison with the reference: b9_mass_hist's (tests/masshist_check.py) -- rtol 1e-9, the project's per-star
tolerance, and, because the kernels prune, atol = N_nodes e^-40 per row on a star entry, times n_stars on a row_cells entry.
Mass edges are separated from every reference node value by 1e-9 relative (masshist_ref.separate_edges).  The catalogues are
synth.make_cluster's with binary_frac = 0.6: about a third of the stars have a true q >= 0.5."""
import ctypes as C
import functools

import numpy as np
import pytest

import masshist_check as hc
import masshist_ref as hr
import moments_ref as mr
import ratiohist_ref as rr
import test_gpu_moments as tm
from base_amd import abi, synth
from cli_util import cli as _cli

pytestmark = pytest.mark.gpu

_dp = C.POINTER(C.c_double)
EVERYTHING = np.array([0.0, np.finfo(float).max])


@functools.lru_cache(maxsize=None)
def problem(name="parsec", n_filt=4, n_stars=70, wd_frac=0.1, n_pops=1, n_y=1, n_eep=90):
    """(pack_d, cl, pack, stars, priors): conftest.build_problem's small pack with a binary-rich catalogue."""
    pack_d = synth.make_pack(name, n_filt=n_filt, n_y=n_y, n_feh=4, n_age=8, n_eep=n_eep)
    truth = synth.default_params(pack_d)
    cl = synth.make_cluster(pack_d, n_stars, seed=12, truth=truth, wd_frac=wd_frac, n_pops=n_pops, binary_frac=0.6)
    return pack_d, cl, abi.make_pack(pack_d), abi.make_stars(cl), synth.default_priors(pack_d, truth, n_pops)


def make_engine(pack, stars, priors, n_pops, K, Q, mode=abi.MODE_GIVEN_MASS, pruning=True):
    from base_amd import engine
    eng = engine.Engine(pack, stars, priors, tm.opts(n_pops, K, Q, mode))
    if not pruning:
        eng.set_tuning(marg_no_pruning=1)
    return eng


def device_cells(pack, stars, priors, n_pops, K, Q, rows, edges, pruning=True):
    eng = make_engine(pack, stars, priors, n_pops, K, Q, pruning=pruning)
    try:
        return eng.ratio_hist(rows, edges)
    finally:
        eng.close()


def mass_edges(nodes, n_mbins):
    """n_mbins + 1 edges with about equal posterior weight per bin, separated from every reference node (masshist_check)."""
    return hc.quantile_edges(nodes, hr.PRIMARY, n_mbins)


def against_reference(pack_d, cl, pack, stars, priors, n_pops, K, Q, rows, edges, nodes, pruning=True):
    got_star, got_rows = device_cells(pack, stars, priors, n_pops, K, Q, rows, edges, pruning)
    want_star, want_rows = rr.reference(pack_d, cl, rows, n_pops, K, Q, edges, nodes)
    print(f"{len(edges) - 1} mass bins x {Q} ratios: largest relative difference among the entries above 1e-6: star_cells "
          f"{hc.largest_rel(got_star, want_star):.3g}, row_cells {hc.largest_rel(got_rows, want_rows):.3g}")
    hc.assert_hist(got_star, got_rows, want_star, want_rows, tm.n_nodes_of(pack_d, n_pops, K, Q), len(cl["mass1"]))
    return got_star, got_rows, want_star, want_rows


@functools.lru_cache(maxsize=None)
def case(n_pops, wd_frac, Q, K=2):
    """dsed, 5 filters, 70 stars, 3 rows + one outside the grid, with the reference's nodes."""
    pack_d, cl, pack, stars, priors = problem("dsed", 5, 70, wd_frac, n_pops, 3 if n_pops == 2 else 1)
    rows = tm.rows_for(pack_d, cl, n_pops)
    rows.setflags(write=False)
    return pack_d, cl, pack, stars, priors, rows, hr.nodes_of_rows(pack_d, cl, rows, n_pops, K, Q)


@functools.lru_cache(maxsize=None)
def small(Q, K=2):
    """parsec, 4 filters, 70 stars (WD-stage among them), one population, 3 rows + one outside."""
    pack_d, cl, pack, stars, priors = problem()
    rows = tm.rows_for(pack_d, cl, 1)
    rows.setflags(write=False)
    return pack_d, cl, pack, stars, priors, rows, hr.nodes_of_rows(pack_d, cl, rows, 1, K, Q)


# ---- 1. parity with the reference -----------------------------------------------------------------------------------------
PARITY = [  # populations, WD-stage fraction, Q, pruning: every value of each, Q below, on and above the four waves of the dealing
    (1, 0.1, 1, True), (1, 0.1, 3, True), (2, 0.1, 4, True), (1, 0.0, 5, True), (2, 0.0, 8, True),
    (1, 0.0, 1, False), (2, 0.1, 3, False), (1, 0.1, 4, False), (2, 0.0, 5, False), (1, 0.1, 8, False),
]


@pytest.mark.parametrize("n_pops,wd_frac,Q,pruning", PARITY, ids=[f"pops{p}-wd{int(w > 0)}-Q{q}-{'pruned' if pr else 'unpruned'}" for p, w, q, pr in PARITY])
def test_parity_with_reference(n_pops, wd_frac, Q, pruning):
    pack_d, cl, pack, stars, priors, rows, nodes = case(n_pops, wd_frac, Q)
    n_mbins = 6
    edges = mass_edges(nodes, n_mbins)
    want_star, _ = rr.reference(pack_d, cl, rows, n_pops, 2, Q, edges, nodes)
    # not vacuous, from the reference alone: mass bins, companion ratios and WD-stage stars carry weight
    cells = want_star[:, :-1].reshape(-1, n_mbins, Q)
    wd = np.asarray(cl["stage"]) == abi.STAGE_WD
    per_bin, per_ratio = cells.sum(axis=(0, 2)), cells.sum(axis=(0, 1))
    print(f"reference: weight per mass bin {per_bin}, per ratio node {per_ratio}, WD-stage {cells[wd].sum():.4g}")
    assert (per_bin > 1e-3).sum() >= 2
    assert Q == 1 or (per_ratio[1:] > 1e-3).sum() >= 2
    assert wd.any() == (wd_frac > 0) and (not wd.any() or cells[wd, :, 0].sum() > 1e-3)
    got_star, got_rows, _, _ = against_reference(pack_d, cl, pack, stars, priors, n_pops, 2, Q, rows, edges, nodes, pruning)
    assert np.all(got_rows[-1] == 0)                                   # the row outside the grid adds nothing
    got_cells = got_star[:, :-1].reshape(-1, n_mbins, Q)
    assert np.all(got_cells[wd, :, 1:] == 0)                           # WD-stage stars: ratio 0 only, the other columns written 0


# ---- 2. edges of the shapes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_wd", [0, 1, 4, 5])
@pytest.mark.parametrize("n_ms", [1, 64, 65])
def test_star_count_edges(n_ms, n_wd):
    pack_d, cl, pack, _, priors = problem(n_stars=400)
    stage = np.asarray(cl["stage"])
    ms, wd = np.flatnonzero(stage != abi.STAGE_WD)[:n_ms], np.flatnonzero(stage == abi.STAGE_WD)[:n_wd]
    assert len(ms) == n_ms and len(wd) == n_wd
    cl = tm.subset(cl, np.sort(np.concatenate([ms, wd])))
    rows = tm.rows_for(pack_d, cl, 1, 2)
    nodes = hr.nodes_of_rows(pack_d, cl, rows, 1, 2, 3)
    against_reference(pack_d, cl, pack, abi.make_stars(cl), priors, 1, 2, 3, rows, mass_edges(nodes, 11 if n_wd % 2 else 5), nodes)


@pytest.mark.parametrize("n_mbins,Q", [(1, 1), (8, 4), (9, 4), (11, 3), (16, 8), (16, 1), (3, 40)])
def test_column_tile_edges(n_mbins, Q):
    """Both sides of the tile seam: 32 columns in one tile (8 x 4), 33 and more in two (9 x 4: 8 + 1 mass bins; 11 x 3: 10 + 1),
    four tiles of 4 mass bins (16 x 8), the one- and sixteen-bin ends at one ratio, and Q above 32: one mass bin a tile."""
    pack_d, cl, pack, stars, priors, rows, nodes = small(Q)
    against_reference(pack_d, cl, pack, stars, priors, 1, 2, Q, rows, mass_edges(nodes, n_mbins), nodes)


@pytest.mark.parametrize("n_eep,K,n_chunks", [(40, 1, 1), (90, 3, 5)])
def test_node_table_edges(n_eep, K, n_chunks):
    """One partial 64-node chunk; five chunks, the last one partial."""
    pack_d, cl, pack, stars, priors = problem(n_eep=n_eep)
    assert ((int(np.max(pack_d["iso_n_eep"])) - 1) * K + 63) // 64 == n_chunks
    rows = tm.rows_for(pack_d, cl, 1)
    nodes = hr.nodes_of_rows(pack_d, cl, rows, 1, K, 3)
    against_reference(pack_d, cl, pack, stars, priors, 1, K, 3, rows, mass_edges(nodes, 9), nodes)


@pytest.mark.parametrize("n_pops", [1, 2])
@pytest.mark.parametrize("n_filt", [4, 8, 16])
def test_every_instance(n_filt, n_pops):
    pack_d, cl, pack, stars, priors = problem("dsed", n_filt, 70, 0.1, n_pops, 3 if n_pops == 2 else 1)
    rows = tm.rows_for(pack_d, cl, n_pops, 2, outside=False)
    nodes = hr.nodes_of_rows(pack_d, cl, rows, n_pops, 2, 3)
    against_reference(pack_d, cl, pack, stars, priors, n_pops, 2, 3, rows, mass_edges(nodes, 11), nodes)


# ---- 3. paths and ranges ------------------------------------------------------------------------------------------------------
def test_rescale_path():
    """Photometry five times sharper: the largest term of most stars lies more than 600 e-folds above the seed (the best of
    every 16th node at mass ratio 0), so the online reference must jump and the LDS columns be rescaled."""
    import numpy_ref
    pack_d, cl, pack, _, priors = problem()
    cl = tm.subset(cl, np.arange(70))
    sig = np.asarray(cl["sigma"], dtype=np.float64)
    cl["sigma"] = np.where(sig > 0, 0.2 * sig, sig)
    rows = tm.rows_for(pack_d, cl, 1, 2, outside=False)
    t, gm, _ = numpy_ref.marg_terms(pack_d, cl, rows[0], 2, 2, 0)
    n_primary = len(gm) // 2
    _, iso_mass, _ = synth.derive_isochrone(pack_d, rows[0][abi.P_LOGAGE], rows[0][abi.P_FEH], rows[0][abi.P_Y])
    assert n_primary == (len(iso_mass) - 1) * 2                          # no empty EEP interval: these are the device's node numbers
    t = np.where(np.isfinite(t), t, -np.inf)
    ms = np.asarray(cl["stage"]) != abi.STAGE_WD
    jump = (t.max(axis=1) - t[:, 0:n_primary:16].max(axis=1))[ms]
    print(f"{(jump > 600).sum()} of {ms.sum()} stars jump by more than 600 e-folds above the seed; the largest jump {jump.max():.4g}")
    assert (jump > 600).sum() >= 40
    nodes = hr.nodes_of_rows(pack_d, cl, rows, 1, 2, 2)
    for n_mbins in (16, 5):
        against_reference(pack_d, cl, pack, abi.make_stars(cl), priors, 1, 2, 2, rows, mass_edges(nodes, n_mbins), nodes)


def test_bin_ranges():
    """Mass edges that hold no node (every cell 0, the totals stand), the nodes of one primary mass only, and every node."""
    Q = 4
    pack_d, cl, pack, stars, priors, rows, nodes = small(Q)
    v, w = hc.reference_values(nodes, hr.PRIMARY)
    empty = np.linspace(v.max() * 2, v.max() * 3, 4)
    got_star, got_rows, _, _ = against_reference(pack_d, cl, pack, stars, priors, 1, 2, Q, rows, empty, nodes)
    assert np.all(got_star[:, :-1] == 0) and np.all(got_rows[:, :-1] == 0) and (got_star[:, -1] > 0).sum() >= 60
    # one primary mass: the unique reference value that carries the most weight, with room to its neighbours
    u = np.unique(v)
    room = np.minimum(np.diff(u, prepend=-np.inf), np.diff(u, append=np.inf)) > 1e-6 * u
    weight = np.array([w[v == x].sum() for x in u]) * room
    m = u[np.argmax(weight)]
    one = np.array([m * (1 - 1e-7), m * (1 + 1e-7)])
    got_star, _, want_star, _ = against_reference(pack_d, cl, pack, stars, priors, 1, 2, Q, rows, one, nodes)
    assert want_star[:, :Q].sum() > 1e-3 and (want_star[:, :Q].sum(axis=1) < 0.9 * want_star[:, Q]).sum() >= 60
    got_star, _, _, _ = against_reference(pack_d, cl, pack, stars, priors, 1, 2, Q, rows, EVERYTHING, nodes)
    np.testing.assert_allclose(got_star[:, :Q].sum(axis=1), got_star[:, Q], rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("stage", ["ms", "wd"])
def test_bin_seam_on_device_bits(stage):
    """m*: a node mass as b9_sample_mass reports it.  A mass edge AT m* has the node in the bin above it; one ulp higher the node's
    weight -- the reference's p sum w over its nodes within 1e-12 relative of m* (every mass ratio of that primary) -- has moved
    to the bin below, ratio by ratio into the same j (or, on the last edge, in from outside); one ulp lower nothing changes, bit
    for bit."""
    Q = 2
    pack_d, cl, pack, stars, priors, rows, nodes = small(Q)
    row = rows[:1]
    want = np.asarray(cl["stage"]) == abi.STAGE_WD if stage == "wd" else np.asarray(cl["stage"]) != abi.STAGE_WD
    eng = make_engine(pack, stars, priors, 1, 2, Q)
    try:
        mass, ratio, member, pop = eng.sample_mass(row, seed=5)
        pick = None
        for i in np.flatnonzero(want & (mass[0] > 0) & (member[0] > 0.5)):
            w, L = mr.weights(nodes[0][i])
            at = np.abs(nodes[0][i][1] - mass[0, i]) <= 1e-12 * mass[0, i]
            if at.any() and w[at].sum() > 1e-3:
                p = mr.membership(cl, i, L)
                pick, moved_ref = i, np.array([p * w[at & (np.rint(nodes[0][i][2] * Q) == j)].sum() for j in range(Q)])
                break
        assert pick is not None
        m = float(mass[0, pick])
        up, down = np.nextafter(m, np.inf), np.nextafter(m, -np.inf)
        a, c = 0.5 * m, 2.0 * m
        h = lambda e: eng.ratio_hist(row, np.array(e))[0]       # noqa: E731
        at_edge, above, below = h([a, m, c]), h([a, up, c]), h([a, down, c])
        assert np.array_equal(below, at_edge)
        tol = 4 * np.finfo(float).eps * (at_edge[pick, :2 * Q].sum())          # the subtractions' own rounding
        print(f"{stage}: star {pick}, m* = {m!r}, moved {above[pick, :Q] - at_edge[pick, :Q]!r}, reference {moved_ref!r}")
        assert moved_ref.sum() > 0 and (stage == "ms" or moved_ref[1:].sum() == 0)
        for j in range(Q):
            assert above[pick, j] - at_edge[pick, j] == pytest.approx(moved_ref[j], rel=1e-9, abs=tol)
            assert at_edge[pick, Q + j] - above[pick, Q + j] == pytest.approx(moved_ref[j], rel=1e-9, abs=tol)
        assert np.array_equal(above[:, 2 * Q], at_edge[:, 2 * Q])
        # the last edge: the node falls out
        out_edge, in_edge, below = h([a, 0.75 * m, m]), h([a, 0.75 * m, up]), h([a, 0.75 * m, down])
        assert np.array_equal(below, out_edge)
        for j in range(Q):
            assert in_edge[pick, Q + j] - out_edge[pick, Q + j] == pytest.approx(moved_ref[j], rel=1e-9, abs=tol)
        assert np.array_equal(in_edge[:, :Q], out_edge[:, :Q]) and np.array_equal(in_edge[:, 2 * Q], out_edge[:, 2 * Q])
    finally:
        eng.close()


# ---- 4. ties to existing calls, on the device -------------------------------------------------------------------------------
def test_ties_to_moments_and_mass_hist():
    pack_d, cl, pack, stars, priors, rows, nodes = case(2, 0.1, 4)
    eng = make_engine(pack, stars, priors, 2, 2, 4)
    try:
        edges = mass_edges(nodes, 16)
        mom = eng.star_moments(rows)
        hist, hist_rows = eng.mass_hist(rows, edges, abi.HQ_PRIMARY)
        star, rws = eng.ratio_hist(rows, edges)
        assert (star[:, -1] > 0).sum() >= 60
        assert np.array_equal(star[:, -1], mom[:, abi.MOM_MEMBER]) and np.array_equal(star[:, -1], hist[:, -1]) and np.array_equal(rws[:, -1], hist_rows[:, -1])
        np.testing.assert_allclose(star[:, :-1].reshape(-1, 16, 4).sum(axis=2), hist[:, :-1], rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(rws[:, :-1].reshape(-1, 16, 4).sum(axis=2), hist_rows[:, :-1], rtol=1e-12, atol=1e-300)
        one, _ = eng.ratio_hist(rows, EVERYTHING)
        assert np.array_equal(one[:, 4], mom[:, abi.MOM_MEMBER])
        np.testing.assert_allclose(one[:, 1:4].sum(axis=1), mom[:, abi.MOM_BINARY], rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose((one[:, :4] * (np.arange(4) / 4.0)).sum(axis=1), mom[:, abi.MOM_Q], rtol=1e-12, atol=1e-300)
        assert (mom[:, abi.MOM_BINARY] > 1e-3).sum() >= 10
    finally:
        eng.close()


@pytest.mark.parametrize("n_pops", [1, 2])
def test_one_ratio_is_mass_hist_to_the_bit(n_pops):
    """marg_n_q = 1: columns 0 .. n_mbins - 1 and the total are b9_mass_hist(PRIMARY)'s star_hist and row_hist, bit for bit."""
    pack_d, cl, pack, stars, priors, rows, nodes = case(n_pops, 0.1, 1)
    eng = make_engine(pack, stars, priors, n_pops, 2, 1)
    try:
        for n_mbins in (16, 3):
            edges = mass_edges(nodes, n_mbins)
            hist, hist_rows = eng.mass_hist(rows, edges, abi.HQ_PRIMARY)
            star, rws = eng.ratio_hist(rows, edges)
            assert (star[:, :-1] > 0).sum() >= 60
            assert np.array_equal(star, hist) and np.array_equal(rws, hist_rows)
    finally:
        eng.close()


# ---- 5. bitwise invariances -------------------------------------------------------------------------------------------------
def test_bitwise_invariances():
    Q, n_pops = 4, 2
    pack_d, cl, pack, stars, priors = problem("dsed", 5, 130, 0.1, 2, 3)
    rows = synth.walker_params(cl["truth"], 40, seed=8, scale=0.3, n_pops=2)
    nodes = hr.nodes_of_rows(pack_d, cl, rows[:2], n_pops, 2, Q)
    edges = mass_edges(nodes, 16)
    eng = make_engine(pack, stars, priors, n_pops, 2, Q)
    try:
        whole, whole_rows = eng.ratio_hist(rows, edges)
        assert (whole[:, -1] > 0).sum() >= 120 and (whole[:, :-1].reshape(-1, 16, Q).sum(axis=(0, 1)) > 1e-3).sum() >= 3
        # 40 rows in one call (two chunks) = 17 + 23 continued
        acc, r0 = eng.ratio_hist(rows[:17], edges)
        acc, r1 = eng.ratio_hist(rows[17:], edges, acc)
        assert np.array_equal(acc, whole) and np.array_equal(np.concatenate([r0, r1]), whole_rows)
        # a repeated call
        again, again_rows = eng.ratio_hist(rows, edges)
        assert np.array_equal(again, whole) and np.array_equal(again_rows, whole_rows)
        # either output alone
        only_star, none = eng.ratio_hist(rows, edges, want_rows=False)
        assert none is None and np.array_equal(only_star, whole)
        none, only_rows = eng.ratio_hist(rows, edges, want_star=False)
        assert none is None and np.array_equal(only_rows, whole_rows)
        # a mass bin alone = the same bin among 16, in any tile (tiles of 8 mass bins at Q = 4)
        for b in (0, 7, 8, 15):
            alone, alone_rows = eng.ratio_hist(rows, edges[b:b + 2])
            assert np.array_equal(alone[:, :Q], whole[:, b * Q:(b + 1) * Q]) and np.array_equal(alone_rows[:, :Q], whole_rows[:, b * Q:(b + 1) * Q])
            assert np.array_equal(alone[:, Q], whole[:, -1]) and np.array_equal(alone_rows[:, Q], whole_rows[:, -1])
        shifted, _ = eng.ratio_hist(rows, edges[5:])                           # bins 8.. of the first call sit in tile 0 here
        assert np.array_equal(shifted[:, :-1], whole[:, 5 * Q:-1])
    finally:
        eng.close()
    # the same 40 rows as 40 one-row calls, each on a fresh context
    acc = None
    for r in range(40):
        eng = make_engine(pack, stars, priors, n_pops, 2, Q)
        try:
            acc, rr_ = eng.ratio_hist(rows[r:r + 1], edges, acc)
        finally:
            eng.close()
        assert np.array_equal(rr_[0], whole_rows[r])
    assert np.array_equal(acc, whole)
    # a star alone = the same star among 130 (an MS/RGB-stage and a WD-stage one, both with weight)
    stage = np.asarray(cl["stage"])
    live = whole[:, :-1].sum(axis=1) > 1e-3
    for i in (int(np.flatnonzero(live & (stage != abi.STAGE_WD))[0]), int(np.flatnonzero(live & (stage == abi.STAGE_WD))[0])):
        eng = make_engine(pack, abi.make_stars(tm.subset(cl, np.array([i]))), priors, n_pops, 2, Q)
        try:
            alone, alone_rows = eng.ratio_hist(rows, edges)
        finally:
            eng.close()
        assert np.array_equal(alone[0], whole[i])


def test_after_every_other_reduction():
    """The call gives the same bits after each of the other eight reductions over a saved chain on the same context."""
    Q = 3
    pack_d, cl, pack, stars, priors, rows, nodes = case(1, 0.1, Q)
    edges = mass_edges(nodes, 11)
    eng = make_engine(pack, stars, priors, 1, 2, Q)
    try:
        first = eng.ratio_hist(rows, edges)
        n, n_wd = eng.n_stars, eng.n_wd_stars()
        assert n_wd >= 3
        star_edges = np.tile(np.linspace(0.05, 9.0, 25), (n, 1))
        wd_edges = np.tile(np.linspace(0.05, 9.0, 9), (n_wd, 1, 1))
        others = [
            lambda: eng.star_moments(rows), lambda: eng.pointwise(rows, tail_len=4), lambda: eng.mass_hist(rows, edges, abi.HQ_SYSTEM),
            lambda: eng.star_bins(rows, star_edges), lambda: eng.phot_resid(rows), lambda: eng.wd_moments(rows, 64),
            lambda: eng.wd_bins(rows, 64, wd_edges, 1 << abi.WQ_ZAMS), lambda: eng.sample_wd_mass(rows, 64, seed=3),
        ]
        for other in others:
            other()
            got = eng.ratio_hist(rows, edges)
            assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1])
    finally:
        eng.close()


@pytest.mark.parametrize("mode", [abi.MODE_GIVEN_MASS, abi.MODE_MARGINALISED])
def test_sampler_blocks_are_untouched(mode):
    from base_amd import mcmc
    pack_d, cl, pack, stars, priors = problem("parsec", 8, 130, 0.1)
    free = np.array(mcmc.DEFAULT_FREE)
    chol = np.diag([mcmc.DEFAULT_STEP[k] for k in free]) * 0.3
    start = synth.walker_params(cl["truth"], 4, seed=2, scale=0.3)
    rows = tm.rows_for(pack_d, cl, 1)
    edges = 0.1 * 80.0 ** (np.arange(9) / 8.0)

    def run(interleave):
        eng = make_engine(pack, stars, priors, 1, 1, 4, mode)
        try:
            lp0 = eng.logpost(start)
            h = eng.mcmc_submit(start, lp0, np.arange(4), free, chol, 11, 0, 6, asynchronous=True)
            if interleave:
                with pytest.raises(Exception) as e:                        # B9_ERR_STATE: a block is outstanding
                    eng.ratio_hist(rows, edges)
                assert e.value.code == abi.B9_ERR_STATE and "outstanding" in str(e.value)
            first = [np.array(x) for x in eng.mcmc_collect(h)[:4]]
            if interleave:
                star, _ = eng.ratio_hist(rows, edges)
                assert (star[:, -1] > 0).sum() >= 100
            h = eng.mcmc_submit(start, lp0, np.arange(4), free, chol, 11, 6, 6, cont=True, asynchronous=True)
            second = [np.array(x) for x in eng.mcmc_collect(h)[:4]]
        finally:
            eng.close()
        return first + second

    for a, b in zip(run(False), run(True)):
        assert np.array_equal(a, b)


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_untouched():
    from base_amd import mcmc
    pack_d, cl, pack, stars, priors, rows, nodes = small(4)
    rows = np.ascontiguousarray(rows)
    good = np.linspace(0.1, 8.0, 19)

    def caller(eng, Q):
        n = eng.n_stars

        def call(n_rows=4, edges=good[:9], n_mbins=8, star=True, rws=True, params=True, ctx=True, have_edges=True):
            edges = np.ascontiguousarray(edges, dtype=np.float64)
            sc, rc = np.full((n, 18 * Q + 1), 7.25), np.full((4, 18 * Q + 1), 7.25)
            code = eng.lib.b9_ratio_hist(eng._ctx if ctx else None, rows.ctypes.data_as(_dp) if params else None, n_rows,
                                         edges.ctypes.data_as(_dp) if have_edges else None, n_mbins, 0,
                                         sc.ctypes.data_as(_dp) if star else None, rc.ctypes.data_as(_dp) if rws else None)
            assert code == abi.B9_OK or (np.all(sc == 7.25) and np.all(rc == 7.25))
            return code
        return call

    eng = make_engine(pack, stars, priors, 1, 2, 4)
    try:
        call = caller(eng, 4)
        assert call() == abi.B9_OK
        assert call(ctx=False) == abi.B9_ERR_INVALID and call(params=False) == abi.B9_ERR_INVALID and call(have_edges=False) == abi.B9_ERR_INVALID
        assert call(n_rows=0) == abi.B9_ERR_INVALID and call(n_rows=-2) == abi.B9_ERR_INVALID
        assert call(star=False, rws=False) == abi.B9_ERR_INVALID
        assert call(n_mbins=0) == abi.B9_ERR_INVALID
        assert call(edges=good[:18], n_mbins=17) == abi.B9_ERR_INVALID
        assert "B9_RH_MAX_MBINS" in eng.lib.b9_last_error(eng._ctx).decode()
        assert call(edges=good[:17], n_mbins=16) == abi.B9_OK                                   # 16 x 4 = 64 cells
        e = good[:9].copy(); e[8] = np.nan
        assert call(edges=e) == abi.B9_ERR_INVALID
        e = good[:9].copy(); e[8] = np.inf
        assert call(edges=e) == abi.B9_ERR_INVALID
        e = good[:9].copy(); e[5] = e[4]
        assert call(edges=e) == abi.B9_ERR_INVALID                                              # two equal
        assert "ascending" in eng.lib.b9_last_error(eng._ctx).decode()
        assert call(edges=good[:9][::-1]) == abi.B9_ERR_INVALID                                 # descending
        assert call(star=False) == abi.B9_OK and call(rws=False) == abi.B9_OK
        # an outstanding sampler block
        free = np.array(mcmc.DEFAULT_FREE)
        chol = np.diag([mcmc.DEFAULT_STEP[k] for k in free]) * 0.3
        start = synth.walker_params(cl["truth"], 4, seed=2, scale=0.3)
        h = eng.mcmc_submit(start, eng.logpost(start), np.arange(4), free, chol, 11, 0, 6, asynchronous=True)
        assert call() == abi.B9_ERR_STATE
        eng.mcmc_collect(h)
        assert call() == abi.B9_OK
    finally:
        eng.close()
    eng = make_engine(pack, stars, priors, 1, 1, 43)                                            # 3 x 43 = 129 cells
    try:
        call = caller(eng, 43)
        assert call(edges=good[:4], n_mbins=3) == abi.B9_ERR_INVALID
        assert "B9_RH_MAX_CELLS" in eng.lib.b9_last_error(eng._ctx).decode()
        assert call(edges=good[:3], n_mbins=2) == abi.B9_OK                                     # 86 cells, one mass bin a tile
    finally:
        eng.close()


# ---- 7. the CLI ---------------------------------------------------------------------------------------------------------------
def test_cli_binary_stats(tmp_path):
    """simCluster (200 stars, half of them binaries) -> scatterCluster -> singlePopMcmc (short, 4 walkers x 100 main-run rows: the
    program passes them in two batches, the second continued) -> binaryStats --qMin 0.5: the three files parse and equal, to
    the bit, the library's tables of Engine.ratio_hist of the same rows in ONE call; the defaults are min(8, 128 / Q) log-spaced
    mass bins over [0.1, M].  The recovered fraction is printed, not asserted: this synthetic case cannot support "the true
    fraction of stars with q >= 0.5 lies within the table's 16-84 band widened by three of its sd" (docs/LABNOTES.md, the
    b9_ratio_hist section, has the figures: true 0.215 = 43 of 200, recovered 0.2664 +/- 0.0012, band 0.2651 .. 0.2678).  At
    Q = 4 the node q = 0.5 is the nearest one for every true ratio in [0.375, 0.625): the grid's own resolution, not the
    chain's spread, sets the difference, and the band of a 400-row chain knows nothing of it."""
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
    r = _cli("simCluster", "--config", y_true, "--nStars", "200", "--percentBinary", "50", "--minMass", "0.4")
    assert r.returncode == 0, r.stderr
    r = _cli("scatterCluster", "--config", y_true, "--sigmaFloor", "0.01", "--sigmaAtLimit", "0.05", "--faintLimit", "45")
    assert r.returncode == 0, r.stderr
    start = truth.copy()
    start[abi.P_LOGAGE] += 0.004; start[abi.P_MOD] += 0.01; start[abi.P_FEH] -= 0.01
    fit = str(tmp_path / "fit")
    y = synth.write_yaml(str(tmp_path / "fit.yaml"), base + ".sim.scatter", root, fit, start, burn=300, run=100, walkers=4)
    r = _cli("singlePopMcmc", "--config", y, "--priorFe_H", repr(float(truth[abi.P_FEH])), "--priorDistMod", repr(float(truth[abi.P_MOD])),
             "--priorAv", repr(float(truth[abi.P_ABS])))
    assert r.returncode == 0, r.stderr
    edges = np.array([0.05, 0.6, 0.9, 1.4, 20.0])
    r = _cli("binaryStats", "--config", y, "--massEdges", ",".join(repr(float(e)) for e in edges), "--qMin", "0.5")
    assert r.returncode == 0, r.stderr
    assert "star rows/s" in r.stderr

    cl = tm._read_phot(base + ".sim.scatter")
    phot_ids = [ln.split()[0] for ln in open(base + ".sim.scatter").read().splitlines()[1:]]
    rows = hostlib.read_res_rows(fit + ".res", start, 3)
    assert len(rows) == 100 * 4                           # more than one batch of 256
    eng = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cl), synth.default_priors(pack_d, truth), tm.opts(1, K, Q))
    try:
        star, rws = eng.ratio_hist(rows, edges)
        m_max = eng.max_mass
    finally:
        eng.close()
    labels, cols, frac = hostlib.read_table_file(fit + ".binaryFraction", "bin")
    assert labels == ["0", "1", "2", "3", "all"] and cols == list(hostlib.BINARY_FRACTION_COLUMNS)
    want = hostlib.binary_table(rws, edges, Q, 0.5)
    assert np.array_equal(frac, want)                    # 17 digits: the chunked pass gives the bits of one call
    labels, cols, dist = hostlib.read_table_file(fit + ".ratioDist", "bin")
    assert labels == [b for b in ("0", "1", "2", "3", "all") for _ in range(Q)] and cols == list(hostlib.RATIO_DIST_COLUMNS)
    assert np.array_equal(dist, hostlib.ratio_dist_table(rws, 4, Q).reshape(-1, 8))
    ids, cols, per = hostlib.read_table_file(fit + ".starRatio", "id")
    assert ids == phot_ids and cols == ["rows", "member", "inRange", "pBinaryAbove"] + [f"q{j}" for j in range(Q)]
    assert np.array_equal(per, hostlib.star_ratio_table(star, 4, Q, len(rows), 0.5))
    # the recovered fraction against the simulated catalogue's own
    q_true = np.asarray(cl["mass_ratio"])
    true_f = float((q_true >= 0.5).mean())
    allf = want[-1]
    print(f"binary fraction at q >= 0.5: true {true_f:.4f} ({int((q_true >= 0.5).sum())} of {len(q_true)}; {int((q_true >= 0.375).sum())} have q >= 0.375, "
          f"nearer to the node 0.5 than to 0.25); recovered mean {allf[8]:.4f} sd {allf[9]:.4f} "
          f"p16 {allf[10]:.4f} p50 {allf[11]:.4f} p84 {allf[12]:.4f}; N mean {allf[3]:.2f}; rows {allf[2]:.0f}")
    assert allf[2] == len(rows) and allf[3] > 100 and 0.0 < allf[10] <= allf[11] <= allf[12] < 1.0

    # the defaults: 8 log-spaced mass bins over [0.1, M], every companion counts
    r = _cli("binaryStats", "--config", y)
    assert r.returncode == 0, r.stderr
    labels, _, frac = hostlib.read_table_file(fit + ".binaryFraction", "bin")
    assert labels == [str(b) for b in range(8)] + ["all"] and frac[0, 0] == 0.1 and frac[7, 1] == m_max and frac[8, 0] == 0.1 and frac[8, 1] == m_max
    np.testing.assert_allclose(frac[:8, 1], 0.1 * (m_max / 0.1) ** (np.arange(1, 9) / 8.0), rtol=1e-14)
    r = _cli("binaryStats", "--config", y, "--massBins", "17")
    assert r.returncode != 0 and "massBins" in r.stderr
