"""b9_mass_hist (the massFunction counterpart) on the GPU: star_hist and row_hist against the numpy statement
tests/masshist_ref.py, the edges of the star, node and bin shapes, the bin seam on the device's own bits, bit-for-bit
invariances, the ties to b9_star_moments, the errors, every kernel instance, and the CLI.  Each test makes its own
short-lived engine on the small packs of build_problem(small=True); a case's reference nodes are computed once and shared.

Tolerance of every comparison with the reference (tests/masshist_check.py): rtol 1e-9 -- the project's per-star tolerance
 -- and, because the kernels prune, atol = N_nodes e^-40 per row on a star entry, times n_stars on a
row_hist entry.  Edges are separated from every reference node value by 1e-9 relative (the device forms M1 by fma, numpy
by two roundings: a node that close to an edge could fall either way)."""
import ctypes as C
import functools

import numpy as np
import pytest

import masshist_check as hc
import masshist_ref as hr
import moments_ref as mr
import test_gpu_moments as tm
from base_amd import abi, synth
from conftest import build_problem
from cli_util import cli as _cli

pytestmark = pytest.mark.gpu

QUANTITIES = [abi.HQ_PRIMARY, abi.HQ_SECONDARY, abi.HQ_SYSTEM]
QNAMES = {abi.HQ_PRIMARY: "primary", abi.HQ_SECONDARY: "secondary", abi.HQ_SYSTEM: "system"}
_dp = C.POINTER(C.c_double)


def make_engine(pack, stars, priors, n_pops, K, Q, mode=abi.MODE_GIVEN_MASS):
    from base_amd import engine
    return engine.Engine(pack, stars, priors, tm.opts(n_pops, K, Q, mode))


def device_hist(pack, stars, priors, n_pops, K, Q, rows, edges, quantity):
    eng = make_engine(pack, stars, priors, n_pops, K, Q)
    try:
        return eng.mass_hist(rows, edges, quantity)
    finally:
        eng.close()


def reference_hist(pack_d, cl, rows, n_pops, K, Q, quantity, edges, nodes=None):
    x = hr.all_increments(pack_d, cl, rows, n_pops, K, Q, quantity, edges, nodes_by_row=nodes)
    return hr.accumulate(x), hr.row_sums(x)


def against_reference(pack_d, cl, pack, stars, priors, n_pops, K, Q, rows, edges, quantity, nodes=None, n_nodes=None):
    got_star, got_rows = device_hist(pack, stars, priors, n_pops, K, Q, rows, edges, quantity)
    want_star, want_rows = reference_hist(pack_d, cl, rows, n_pops, K, Q, quantity, edges, nodes)
    print(f"{QNAMES[quantity]}, {len(edges) - 1} bins: largest relative difference among the entries above 1e-6: star_hist {hc.largest_rel(got_star, want_star):.3g}, "
          f"row_hist {hc.largest_rel(got_rows, want_rows):.3g}")
    hc.assert_hist(got_star, got_rows, want_star, want_rows, n_nodes or tm.n_nodes_of(pack_d, n_pops, K, Q), len(cl["mass1"]))
    return got_star, got_rows, want_star, want_rows


@functools.lru_cache(maxsize=None)
def case(k):
    """Case k of test_gpu_moments.CASES with its rows (3 + one outside the grid) and the reference's nodes, built once."""
    name, n_filt, n_y, n_pops, K, Q, n_stars, wd_frac, n_nodes = tm.CASES[k]
    pack_d, cl, pack, stars, priors, _ = build_problem(name, n_filt, n_stars=n_stars, wd_frac=wd_frac, n_y=n_y, n_pops=n_pops, seed=12)
    rows = tm.rows_for(pack_d, cl, n_pops)
    rows.setflags(write=False)
    return pack_d, cl, pack, stars, priors, rows, hr.nodes_of_rows(pack_d, cl, rows, n_pops, K, Q)


@functools.lru_cache(maxsize=None)
def small():
    """parsec, 4 filters, 70 stars (WD-stage among them), one population, 2 x 2 grid, 3 rows + one outside."""
    pack_d, cl, pack, stars, priors, _ = build_problem("parsec", 4, n_stars=70, wd_frac=0.1, seed=12)
    rows = tm.rows_for(pack_d, cl, 1)
    rows.setflags(write=False)
    return pack_d, cl, pack, stars, priors, rows, hr.nodes_of_rows(pack_d, cl, rows, 1, 2, 2)


# ---- 1. parity with the reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("quantity", QUANTITIES, ids=[QNAMES[q] for q in QUANTITIES])
@pytest.mark.parametrize("k", range(4), ids=[f"{c[0]}{c[1]}" for c in tm.CASES])
def test_parity_with_reference(k, quantity):
    """64 bins (two tiles) holding about equal posterior weight each.  Non-vacuity, from the reference alone (figures of
    the reference: stars with two or more bins above 1e-3 of their total / live stars, PRIMARY SECONDARY SYSTEM -- dsed 5:
    114 80 121 / 127; parsec 8: 104 92 117 / 123; girardi 3 (one mass ratio: no companions): 67 0 67 / 69; parsec 9 (a
    single companion ratio): 57 27 56 / 67.  Stars whose mean membership lies inside (0.01, 0.99): 1, 32, 0, 21 -- the
    catalogues' membership is saturated except in the second case, where the bound is asserted, as the moments suite does)."""
    name, n_filt, n_y, n_pops, K, Q, n_stars, wd_frac, n_nodes = tm.CASES[k]
    pack_d, cl, pack, stars, priors, rows, nodes = case(k)
    edges = hc.quantile_edges(nodes, quantity, 64)
    v, _ = hc.reference_values(nodes, quantity)
    if len(v):                                           # no reference node value within 1e-9 relative of an edge
        near = np.abs(v[:, None] - edges[None, :]) <= 1e-9 * np.abs(edges[None, :])
        assert not near.any()
    got_star, got_rows, want_star, want_rows = against_reference(pack_d, cl, pack, stars, priors, n_pops, K, Q, rows, edges, quantity, nodes, n_nodes)
    assert np.all(got_rows[-1] == 0)                                   # the row outside the grid adds nothing
    live, two, inside = hc.non_vacuity(want_star, 3)
    print(f"{name} {n_filt} {QNAMES[quantity]}: {live} live, {two} with two or more bins, {inside} with membership inside")
    if quantity != abi.HQ_SECONDARY or k < 2:
        assert two >= (live + 1) // 2
    if k == 1:
        assert inside >= 25
    if quantity == abi.HQ_SECONDARY:
        wd = np.asarray(cl["stage"]) == abi.STAGE_WD
        assert np.all(got_star[wd, :64] == 0) and (not wd.any() or np.any(got_star[wd, 64] > 0))


# ---- 2. edges of the shapes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_wd", [0, 1, 4, 5])
@pytest.mark.parametrize("n_ms", [1, 64, 65])
def test_star_count_edges(n_ms, n_wd):
    pack_d, cl, pack, _, priors, _ = build_problem("parsec", 4, n_stars=400, wd_frac=0.1, seed=12)
    stage = np.asarray(cl["stage"])
    ms, wd = np.flatnonzero(stage != abi.STAGE_WD)[:n_ms], np.flatnonzero(stage == abi.STAGE_WD)[:n_wd]
    assert len(ms) == n_ms and len(wd) == n_wd
    cl = tm.subset(cl, np.sort(np.concatenate([ms, wd])))
    rows = tm.rows_for(pack_d, cl, 1, 2)
    nodes = hr.nodes_of_rows(pack_d, cl, rows, 1, 2, 2)
    quantity = QUANTITIES[(n_ms + n_wd) % 3]
    edges = hc.quantile_edges(nodes, quantity, 33 if n_wd % 2 else 24)
    against_reference(pack_d, cl, pack, abi.make_stars(cl), priors, 1, 2, 2, rows, edges, quantity, nodes)


@pytest.mark.parametrize("n_bins", [1, 32, 33, 64])
def test_bin_count_edges(n_bins):
    """Both sides of the tile seam (32 bins a tile), one and two populations."""
    pack_d, cl, pack, stars, priors, rows, nodes = small()
    for quantity in QUANTITIES:
        against_reference(pack_d, cl, pack, stars, priors, 1, 2, 2, rows, hc.quantile_edges(nodes, quantity, n_bins), quantity, nodes)
    pack_d, cl, pack, stars, priors, rows, nodes = case(0)
    against_reference(pack_d, cl, pack, stars, priors, 2, 2, 2, rows, hc.quantile_edges(nodes, abi.HQ_SYSTEM, n_bins), abi.HQ_SYSTEM, nodes, 712)


def test_bin_ranges():
    """A bin range that holds no node (all bins 0, the totals stand); a range that misses part of the grid (the totals exceed
    the bins' sums)."""
    pack_d, cl, pack, stars, priors, rows, nodes = small()
    v, _ = hc.reference_values(nodes, abi.HQ_PRIMARY)
    empty = np.linspace(v.max() * 2, v.max() * 3, 9)
    got_star, got_rows, want_star, _ = against_reference(pack_d, cl, pack, stars, priors, 1, 2, 2, rows, empty, abi.HQ_PRIMARY, nodes)
    assert np.all(got_star[:, :8] == 0) and np.all(got_rows[:, :8] == 0) and (got_star[:, 8] > 0).sum() >= 60
    full = hc.quantile_edges(nodes, abi.HQ_PRIMARY, 24)
    part = full[8:17]
    got_star, got_rows, want_star, _ = against_reference(pack_d, cl, pack, stars, priors, 1, 2, 2, rows, part, abi.HQ_PRIMARY, nodes)
    assert (want_star[:, :8].sum(axis=1) < 0.5 * want_star[:, 8]).sum() >= 20      # (the reference's own figures)
    assert (got_star[:, :8].sum(axis=1) < 0.5 * got_star[:, 8]).sum() >= 20


def test_special_stars():
    """A star with every filter unused, one with (all but) no membership prior, one with membership prior 1.  b9_load_stars
    takes clust_prior in (0, 1] only (tests/test_gpu_moments.py checks the refusal), so the star without membership prior
    carries 1e-300: every entry of it is 0 to every tolerance."""
    pack_d, cl, pack, _, priors, _ = build_problem("parsec", 4, n_stars=70, wd_frac=0.1, seed=12)
    cl = tm.subset(cl, np.arange(70))
    cl["sigma"] = np.array(cl["sigma"], dtype=np.float64)
    cl["clust_prior"] = np.array(cl["clust_prior"], dtype=np.float64)
    ms = np.flatnonzero(np.asarray(cl["stage"]) != abi.STAGE_WD)
    cl["sigma"][ms[3]] = -1.0
    cl["clust_prior"][ms[5]] = 1e-300
    cl["clust_prior"][ms[7]] = 1.0
    rows = tm.rows_for(pack_d, cl, 1)
    nodes = hr.nodes_of_rows(pack_d, cl, rows, 1, 2, 2)
    edges = hc.quantile_edges(nodes, abi.HQ_PRIMARY, 24)
    got, _, want, _ = against_reference(pack_d, cl, pack, abi.make_stars(cl), priors, 1, 2, 2, rows, edges, abi.HQ_PRIMARY, nodes)
    assert np.all(got[ms[5]] < 1e-250)
    assert got[ms[7], 24] == 3.0
    assert got[ms[3], 24] > 0 and (got[ms[3], :24] > 0).sum() >= 12            # no photometry: the prior over the whole grid


def test_rescale_path():
    """Photometry five times sharper: the largest term of most stars lies more than 600 e-folds above the seed (the best of
    every 16th node at mass ratio 0), so the online reference must jump and the LDS bins be rescaled."""
    import numpy_ref
    pack_d, cl, pack, _, priors, _ = build_problem("parsec", 4, n_stars=70, wd_frac=0.1, seed=12)
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
    for quantity, n_bins in ((abi.HQ_PRIMARY, 64), (abi.HQ_SYSTEM, 24)):
        against_reference(pack_d, cl, pack, abi.make_stars(cl), priors, 1, 2, 2, rows, hc.quantile_edges(nodes, quantity, n_bins), quantity, nodes)


@pytest.mark.parametrize("n_eep,K,n_chunks", [(40, 1, 1), (90, 3, 5)])
def test_node_table_edges(n_eep, K, n_chunks):
    """One partial 64-node chunk; five chunks, the last one partial."""
    pack_d, cl, pack, stars, priors, _ = build_problem("parsec", 4, n_stars=70, wd_frac=0.1, seed=12, n_eep=n_eep)
    assert ((int(np.max(pack_d["iso_n_eep"])) - 1) * K + 63) // 64 == n_chunks
    rows = tm.rows_for(pack_d, cl, 1)
    nodes = hr.nodes_of_rows(pack_d, cl, rows, 1, K, 2)
    against_reference(pack_d, cl, pack, stars, priors, 1, K, 2, rows, hc.quantile_edges(nodes, abi.HQ_SYSTEM, 33), abi.HQ_SYSTEM, nodes)


@pytest.mark.parametrize("n_pops", [1, 2])
@pytest.mark.parametrize("n_filt", [4, 8, 16])
def test_every_instance(n_filt, n_pops):
    pack_d, cl, pack, stars, priors, _ = build_problem("dsed", n_filt, n_stars=70, wd_frac=0.1, n_y=3 if n_pops == 2 else 1, n_pops=n_pops, seed=12)
    rows = tm.rows_for(pack_d, cl, n_pops, 2, outside=False)
    nodes = hr.nodes_of_rows(pack_d, cl, rows, n_pops, 2, 2)
    against_reference(pack_d, cl, pack, stars, priors, n_pops, 2, 2, rows, hc.quantile_edges(nodes, abi.HQ_PRIMARY, 40), abi.HQ_PRIMARY, nodes)


# ---- 3. the bin seam on the device's own bits -------------------------------------------------------------------------------
@pytest.mark.parametrize("stage", ["ms", "wd"])
def test_bin_seam_on_device_bits(stage):
    """m*: a node mass as b9_sample_mass reports it.  An edge AT m* has the node in the bin above it; one ulp higher the node's
    weight -- the reference's p sum w over its nodes within 1e-12 relative of m* (every mass ratio of that primary) -- has moved
    to the bin below (or, on the last edge, in from outside); one ulp lower nothing changes, bit for bit."""
    pack_d, cl, pack, stars, priors, rows, nodes = small()
    row = rows[:1]
    want = np.asarray(cl["stage"]) == abi.STAGE_WD if stage == "wd" else np.asarray(cl["stage"]) != abi.STAGE_WD
    eng = make_engine(pack, stars, priors, 1, 2, 2)
    try:
        mass, ratio, member, pop = eng.sample_mass(row, seed=5)
        # the star: of the wanted stage, a member, drawn at a node that carries at least 1e-3 of its posterior
        pick = None
        for i in np.flatnonzero(want & (mass[0] > 0) & (member[0] > 0.5)):
            w, L = mr.weights(nodes[0][i])
            at = np.abs(nodes[0][i][1] - mass[0, i]) <= 1e-12 * mass[0, i]
            if at.any() and w[at].sum() > 1e-3:
                pick, moved_ref = i, mr.membership(cl, i, L) * w[at].sum()
                break
        assert pick is not None
        m = float(mass[0, pick])
        up, down = np.nextafter(m, np.inf), np.nextafter(m, -np.inf)
        a, c = 0.5 * m, 2.0 * m
        h = lambda e: eng.mass_hist(row, np.array(e), abi.HQ_PRIMARY)[0]       # noqa: E731
        at_edge, above, below = h([a, m, c]), h([a, up, c]), h([a, down, c])
        assert np.array_equal(below, at_edge)
        moved = above[pick, 0] - at_edge[pick, 0]
        tol = 4 * np.finfo(float).eps * (at_edge[pick, 0] + at_edge[pick, 1])   # the subtraction's own rounding
        print(f"{stage}: star {pick}, m* = {m!r}, moved {moved!r}, reference {moved_ref!r}")
        assert moved == pytest.approx(moved_ref, rel=1e-9, abs=tol)
        assert at_edge[pick, 1] - above[pick, 1] == pytest.approx(moved_ref, rel=1e-9, abs=tol)
        assert np.array_equal(above[:, 2], at_edge[:, 2])
        # the last edge: the node falls out
        out_edge, in_edge, below = h([a, 0.75 * m, m]), h([a, 0.75 * m, up]), h([a, 0.75 * m, down])
        assert np.array_equal(below, out_edge)
        assert in_edge[pick, 1] - out_edge[pick, 1] == pytest.approx(moved_ref, rel=1e-9, abs=tol)
        assert np.array_equal(in_edge[:, 0], out_edge[:, 0]) and np.array_equal(in_edge[:, 2], out_edge[:, 2])
    finally:
        eng.close()


# ---- 4. bitwise invariances -------------------------------------------------------------------------------------------------
def test_bitwise_invariances():
    pack_d, cl, pack, stars, priors, _, nodes = case(0)
    rows = synth.walker_params(cl["truth"], 40, seed=8, scale=0.3, n_pops=2)
    outside = rows[0].copy(); outside[abi.P_LOGAGE] = pack_d["log_age"][-1] + 1.0
    edges = hc.quantile_edges(nodes, abi.HQ_PRIMARY, 64)
    q = abi.HQ_PRIMARY
    eng = make_engine(pack, stars, priors, 2, 2, 2)
    try:
        whole, whole_rows = eng.mass_hist(rows, edges, q)
        assert (whole[:, 64] > 0).sum() >= 120
        # a bin alone = the same bin among 63 others, in either tile
        for b in (3, 31, 32, 50):
            alone, alone_rows = eng.mass_hist(rows, edges[b:b + 2], q)
            assert np.array_equal(alone[:, 0], whole[:, b]) and np.array_equal(alone_rows[:, 0], whole_rows[:, b])
            assert np.array_equal(alone[:, 1], whole[:, 64]) and np.array_equal(alone_rows[:, 1], whole_rows[:, 64])
        shifted, _ = eng.mass_hist(rows, edges[20:], q)                        # bins 32.. of the first call sit in tile 0 here
        assert np.array_equal(shifted[:, :44], whole[:, 20:64])
        # 40 rows in one call (two chunks) = the same rows as 1 + 32 + 7 continued = chunked by hand into 8s
        acc, r0 = eng.mass_hist(rows[:1], edges, q)
        acc, r1 = eng.mass_hist(rows[1:33], edges, q, acc)
        acc, r2 = eng.mass_hist(rows[33:], edges, q, acc)
        assert np.array_equal(acc, whole) and np.array_equal(np.concatenate([r0, r1, r2]), whole_rows)
        acc = None
        for r in range(0, 40, 8):
            acc, rr = eng.mass_hist(rows[r:r + 8], edges, q, acc)
            assert np.array_equal(rr, whole_rows[r:r + 8])
        assert np.array_equal(acc, whole)
        # a row's line alone = the same row in any position of a batch
        j = 17
        alone, alone_row = eng.mass_hist(rows[j:j + 1], edges, q)
        assert np.array_equal(alone_row[0], whole_rows[j])
        batch = np.tile(outside, (36, 1)); batch[35] = rows[j]
        got, got_rows = eng.mass_hist(batch, edges, q, np.zeros_like(alone))
        assert np.array_equal(got_rows[35], whole_rows[j]) and np.all(got_rows[:35] == 0) and np.array_equal(got, alone)
        # star_hist is the same whether row_hist is NULL or not, and the other way round
        only_star, none = eng.mass_hist(rows, edges, q, want_rows=False)
        assert none is None and np.array_equal(only_star, whole)
        none, only_rows = eng.mass_hist(rows, edges, q, want_star=False)
        assert none is None and np.array_equal(only_rows, whole_rows)
        # a repeated call; the other quantities in between leave nothing behind
        eng.mass_hist(rows[:5], edges[:10], abi.HQ_SYSTEM)
        again, again_rows = eng.mass_hist(rows, edges, q)
        assert np.array_equal(again, whole) and np.array_equal(again_rows, whole_rows)
    finally:
        eng.close()
    eng = make_engine(pack, stars, priors, 2, 2, 2)                           # a fresh context
    try:
        fresh, fresh_rows = eng.mass_hist(rows, edges, q)
        assert np.array_equal(fresh, whole) and np.array_equal(fresh_rows, whole_rows)
    finally:
        eng.close()


@pytest.mark.parametrize("mode", [abi.MODE_GIVEN_MASS, abi.MODE_MARGINALISED])
def test_sampler_blocks_are_untouched(mode):
    from base_amd import mcmc
    pack_d, cl, pack, stars, priors, _, nodes = case(1)
    free = np.array(mcmc.DEFAULT_FREE)
    chol = np.diag([mcmc.DEFAULT_STEP[k] for k in free]) * 0.3
    start = synth.walker_params(cl["truth"], 4, seed=2, scale=0.3)
    rows = tm.rows_for(pack_d, cl, 1)
    edges = hc.quantile_edges(nodes, abi.HQ_PRIMARY, 40)

    def run(interleave):
        eng = make_engine(pack, stars, priors, 1, 1, 4, mode)
        try:
            lp0 = eng.logpost(start)
            h = eng.mcmc_submit(start, lp0, np.arange(4), free, chol, 11, 0, 6, asynchronous=True)
            if interleave:
                with pytest.raises(Exception) as e:                        # B9_ERR_STATE: a block is outstanding
                    eng.mass_hist(rows, edges)
                assert e.value.code == abi.B9_ERR_STATE and "outstanding" in str(e.value)
            first = [np.array(x) for x in eng.mcmc_collect(h)[:4]]
            if interleave:
                star, _ = eng.mass_hist(rows, edges)
                assert (star[:, 40] > 0).sum() >= 100
            h = eng.mcmc_submit(start, lp0, np.arange(4), free, chol, 11, 6, 6, cont=True, asynchronous=True)
            second = [np.array(x) for x in eng.mcmc_collect(h)[:4]]
        finally:
            eng.close()
        return first + second

    for a, b in zip(run(False), run(True)):
        assert np.array_equal(a, b)


# ---- 5. ties to existing calls, on the device -------------------------------------------------------------------------------
def test_ties_to_star_moments():
    pack_d, cl, pack, stars, priors, rows, nodes = case(0)
    eng = make_engine(pack, stars, priors, 2, 2, 2)
    try:
        mom = eng.star_moments(rows)
        everything = np.array([0.0, np.finfo(float).max])
        star, rws = eng.mass_hist(rows, everything, abi.HQ_PRIMARY)
        np.testing.assert_allclose(star[:, 1], mom[:, abi.MOM_MEMBER], rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(star[:, 0], mom[:, abi.MOM_MEMBER], rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(rws[:, 1].sum(), mom[:, abi.MOM_MEMBER].sum(), rtol=1e-12)
        sec, _ = eng.mass_hist(rows, everything, abi.HQ_SECONDARY)
        np.testing.assert_allclose(sec[:, 0], mom[:, abi.MOM_BINARY], rtol=1e-12, atol=1e-300)
        # 64 narrow bins over the catalogue's masses bracket the mean primary mass within a bin's width
        v, _ = hc.reference_values(nodes, abi.HQ_PRIMARY)
        lo, hi = v.min() * 0.999, v.max() * 1.001
        edges = np.linspace(lo, hi, 65)
        narrow, _ = eng.mass_hist(rows, edges, abi.HQ_PRIMARY)
        np.testing.assert_allclose(narrow[:, :64].sum(axis=1), mom[:, abi.MOM_MEMBER], rtol=1e-12, atol=1e-300)
        centre, width = 0.5 * (edges[:-1] + edges[1:]), (hi - lo) / 64
        live = mom[:, abi.MOM_MEMBER] > 0
        mean_binned = (narrow[live, :64] * centre).sum(axis=1) / mom[live, abi.MOM_MEMBER]
        mean_exact = mom[live, abi.MOM_M1] / mom[live, abi.MOM_MEMBER]
        assert live.sum() >= 100 and np.all(np.abs(mean_binned - mean_exact) <= 0.5 * width * (1 + 1e-9))
    finally:
        eng.close()


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_untouched():
    from base_amd import mcmc
    pack_d, cl, pack, stars, priors, rows, nodes = small()
    eng = make_engine(pack, stars, priors, 1, 2, 2)
    try:
        n = eng.n_stars
        rows = np.ascontiguousarray(rows)
        good = np.linspace(0.1, 8.0, 66)

        def call(n_rows=4, quantity=abi.HQ_PRIMARY, edges=good[:25], n_bins=24, star=True, rws=True, params=True):
            edges = np.ascontiguousarray(edges, dtype=np.float64)
            sh, rh = np.full((n, 66), 7.25), np.full((4, 66), 7.25)
            rc = eng.lib.b9_mass_hist(eng._ctx, rows.ctypes.data_as(_dp) if params else None, n_rows, quantity, edges.ctypes.data_as(_dp), n_bins, 0,
                                      sh.ctypes.data_as(_dp) if star else None, rh.ctypes.data_as(_dp) if rws else None)
            assert rc == abi.B9_OK or (np.all(sh == 7.25) and np.all(rh == 7.25))
            return rc

        assert call() == abi.B9_OK
        assert call(n_bins=0) == abi.B9_ERR_INVALID
        assert call(edges=good, n_bins=65) == abi.B9_ERR_INVALID
        assert call(edges=good[:25][::-1]) == abi.B9_ERR_INVALID                               # descending
        e = good[:25].copy(); e[10] = e[9]
        assert call(edges=e) == abi.B9_ERR_INVALID                                              # two equal
        e = good[:25].copy(); e[24] = np.nan
        assert call(edges=e) == abi.B9_ERR_INVALID
        e = good[:25].copy(); e[24] = np.inf
        assert call(edges=e) == abi.B9_ERR_INVALID
        assert call(quantity=3) == abi.B9_ERR_INVALID and call(quantity=-1) == abi.B9_ERR_INVALID
        assert call(n_rows=0) == abi.B9_ERR_INVALID and call(n_rows=-2) == abi.B9_ERR_INVALID
        assert call(star=False, rws=False) == abi.B9_ERR_INVALID
        assert call(params=False) == abi.B9_ERR_INVALID
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


# ---- 7. the CLI ---------------------------------------------------------------------------------------------------------------
def test_cli_mass_function(tmp_path):
    """simCluster (200 stars) -> scatterCluster -> singlePopMcmc (short, 4 walkers x 100 main-run rows: the program passes
    them in two batches, the second continued) -> massFunction --perStar: both files equal, to the printed precision, what
    Engine.mass_hist in ONE call gives through the reference table (tests/masshist_ref.table); the defaults are 24
    log-spaced bins over [0.1, M_wd_up]; a second run with other flags is read back as well."""
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
    y = synth.write_yaml(str(tmp_path / "fit.yaml"), base + ".sim.scatter", root, fit, start, burn=300, run=100, walkers=4)
    r = _cli("singlePopMcmc", "--config", y, "--priorFe_H", repr(float(truth[abi.P_FEH])), "--priorDistMod", repr(float(truth[abi.P_MOD])),
             "--priorAv", repr(float(truth[abi.P_ABS])))
    assert r.returncode == 0, r.stderr
    r = _cli("massFunction", "--config", y, "--perStar")
    assert r.returncode == 0, r.stderr
    assert "star rows/s" in r.stderr

    cl = tm._read_phot(base + ".sim.scatter")
    phot_ids = [ln.split()[0] for ln in open(base + ".sim.scatter").read().splitlines()[1:]]
    rows = hostlib.read_res_rows(fit + ".res", start, 3)
    assert len(rows) == 100 * 4                           # more than one batch of 256
    m_up = float(pack_d["m_wd_up"])
    edges = hostlib.mass_function_settings(["--config", y], m_wd_up=m_up)[1]
    assert len(edges) == 25 and edges[0] == 0.1 and edges[-1] == m_up
    eng = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cl), synth.default_priors(pack_d, truth), tm.opts(1, K, Q))
    try:
        star, rws = eng.mass_hist(rows, edges, abi.HQ_PRIMARY)
        flags2 = ["--nBins", "10", "--minMass", "0.3", "--maxMass", "3.0", "--linearBins", "--quantity", "system"]
        edges2 = hostlib.mass_function_settings(["--config", y] + flags2, m_wd_up=m_up)[1]
        np.testing.assert_allclose(edges2, np.linspace(0.3, 3.0, 11), rtol=1e-14)
        _, rws2 = eng.mass_hist(rows, edges2, abi.HQ_SYSTEM)
    finally:
        eng.close()
    _, cols, tab = hostlib.read_table_file(fit + ".massFunction", None)
    assert cols == list(hostlib.MASS_FUNCTION_COLUMNS)
    want = hr.table(rws, edges)
    np.testing.assert_allclose(tab, want, rtol=0, atol=6e-7)               # %.6f
    assert want[:, 2].sum() > 50                                           # most of the 200 stars are members with a mass in range
    # the chunked pass gives the bits of one call: the file's numbers are those of the one-call table printed the same way
    assert [f"{x:.6f}" for x in hostlib.mass_function_table(rws, edges).ravel()] == open(fit + ".massFunction").read().split()[8:]
    ids, cols, per = hostlib.read_table_file(fit + ".starMassHist", "id")
    assert ids == phot_ids and cols == ["rows", "member"] + [f"bin{b}" for b in range(24)]
    tot = star[:, 24]
    want_per = np.concatenate([np.full((len(ids), 1), float(len(rows))), (tot / len(rows))[:, None],
                               np.where(tot[:, None] > 0, star[:, :24] / np.where(tot > 0, tot, 1.0)[:, None], 0.0)], axis=1)
    assert [f"{x:.6f}" for x in want_per[:, 1:].ravel()] == [t for ln in open(fit + ".starMassHist").read().splitlines()[1:] for t in ln.split()[2:]]
    assert np.array_equal(per[:, 0], want_per[:, 0])

    r = _cli("massFunction", "--config", y, *flags2)
    assert r.returncode == 0, r.stderr
    _, _, tab2 = hostlib.read_table_file(fit + ".massFunction", None)
    np.testing.assert_allclose(tab2, hr.table(rws2, edges2), rtol=0, atol=6e-7)
