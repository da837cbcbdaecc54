"""b9_filter_loo (the filterCheck counterpart) on the GPU: star_loo and row_loo against the numpy statement tests/loo_ref.py,
every instance and the filter-tile seam, the edges of the star and node shapes, special stars, promotion and the rescale
path, the route the library had before (reloading the catalogue with one band disabled), the ties to b9_star_moments and
b9_phot_resid, bit-for-bit invariances, the scratch rule, the sampler left alone, the errors, and the CLI.  Each test makes its own
short-lived engine on the small packs of build_problem(small=True); a case's reference is computed once and shared.

Tolerances: tests/loo_check.py (rtol 1e-9 + the pruning's bound per column + the cancellation term of the first moments; for
p l_f 1e-9 p max(1, |L|, |L^f|) + the pruning's bound; with b9_tuning.marg_no_pruning the pruning's bound is dropped)."""
import ctypes as C
import functools

import numpy as np
import pytest

import loo_check as lc
import loo_ref as lr
import moments_ref as mr
import test_gpu_moments as tm
from base_amd import abi, synth
from conftest import build_problem

pytestmark = pytest.mark.gpu
_dp = C.POINTER(C.c_double)


def make_engine(pack, stars, priors, n_pops, K, Q, mode=abi.MODE_GIVEN_MASS):
    from base_amd import engine
    return engine.Engine(pack, stars, priors, tm.opts(n_pops, K, Q, mode))


def against_reference(pack_d, cl, pack, stars, priors, n_pops, K, Q, rows, nodes=None, n_nodes=None, ref=None):
    """Both outputs, with the pruning and without it, against the reference; returns (got_star, got_rows, want_star, want_rows)."""
    n_nodes = n_nodes or tm.n_nodes_of(pack_d, n_pops, K, Q)
    want_star, want_rows, x, bound, absx = ref or lr.reference(pack_d, cl, rows, n_pops, K, Q, nodes)
    eng = make_engine(pack, stars, priors, n_pops, K, Q)
    try:
        got_star, got_rows = eng.filter_loo(rows)
        eng.set_tuning(marg_no_pruning=1)
        full_star, full_rows = eng.filter_loo(rows)
        eng.set_tuning()
    finally:
        eng.close()
    print(f"largest relative difference among the entries above 1e-6: star_loo {lc.largest_rel(got_star, want_star):.3g} "
          f"(unpruned {lc.largest_rel(full_star, want_star):.3g}), row_loo {lc.largest_rel(got_rows, want_rows):.3g} "
          f"(unpruned {lc.largest_rel(full_rows, want_rows):.3g})")
    sig = cl["sigma"]
    lc.assert_star_loo(got_star, want_star, lc.star_atol(bound, absx, n_nodes))
    lc.assert_row_loo(got_rows, want_rows, lc.row_atol(bound, absx, sig, n_nodes))
    lc.assert_variances(got_star, want_star)
    lc.assert_star_loo(full_star, want_star, lc.star_atol(bound, absx, n_nodes, pruning=False))
    lc.assert_row_loo(full_rows, want_rows, lc.row_atol(bound, absx, sig, n_nodes, pruning=False))
    lc.assert_variances(full_star, want_star)
    return got_star, got_rows, want_star, want_rows


@functools.lru_cache(maxsize=None)
def case(k):
    """Case k of test_gpu_moments.CASES with its rows (3 + one outside the grid) and the reference, built once."""
    name, n_filt, n_y, n_pops, K, Q, n_stars, wd_frac, n_nodes = tm.CASES[k]
    pack_d, cl, pack, stars, priors, _ = build_problem(name, n_filt, n_stars=n_stars, wd_frac=wd_frac, n_y=n_y, n_pops=n_pops, seed=12)
    rows = tm.rows_for(pack_d, cl, n_pops)
    rows.setflags(write=False)
    nodes = [mr.star_nodes(pack_d, cl, par, n_pops, K, Q) for par in rows]
    return pack_d, cl, pack, stars, priors, rows, nodes, lr.reference(pack_d, cl, rows, n_pops, K, Q, nodes)


@functools.lru_cache(maxsize=None)
def small():
    """parsec, 4 filters, 70 stars (WD-stage among them), one population, 2 x 2 grid, 3 rows + one outside."""
    pack_d, cl, pack, stars, priors, _ = build_problem("parsec", 4, n_stars=70, wd_frac=0.1, seed=12)
    rows = tm.rows_for(pack_d, cl, 1)
    rows.setflags(write=False)
    return pack_d, cl, pack, stars, priors, rows


# ---- 1. parity with the reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(4), ids=[f"{c[0]}{c[1]}" for c in tm.CASES])
def test_parity_with_reference(k):
    name, n_filt, n_y, n_pops, K, Q, n_stars, wd_frac, n_nodes = tm.CASES[k]
    pack_d, cl, pack, stars, priors, rows, nodes, ref = case(k)
    live = int((ref[0][:, 1] > 0).sum())
    print(f"{name} {n_filt}: {live} live stars")
    assert live >= (n_stars * 6) // 10
    got_star, got_rows, want_star, want_rows = against_reference(pack_d, cl, pack, stars, priors, n_pops, K, Q, rows, nodes, n_nodes, ref)
    assert np.all(got_rows[-1] == 0) and np.all(got_star[got_star[:, 0] > 0, 0] == 3)      # the row outside the grid adds nothing
    assert got_star.shape == (n_stars, 2 + 3 * n_filt) and got_rows.shape == (4, 1 + 6 * n_filt)


# ---- 2. every instance ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pops", [1, 2])
@pytest.mark.parametrize("n_filt", [1, 2, 4, 5, 8, 9, 16])
def test_every_instance(n_filt, n_pops):
    """The six instances; 1 filter (the prior alone predicts it), 2, 5 and 9 filters: padded rows on both sides of the 4 | 8 | 16
    seams.  The 16-filter instances tile the leave-outs 8 + 8 over gridDim.z: 9 filters put one real filter and seven padded ones
    in the second tile, 16 fill both."""
    pack_d, cl, pack, stars, priors, _ = build_problem("dsed", n_filt, n_stars=70, wd_frac=0.1, n_y=3 if n_pops == 2 else 1, n_pops=n_pops, seed=12)
    rows = tm.rows_for(pack_d, cl, n_pops, 2, outside=False)
    got_star, got_rows, _, _ = against_reference(pack_d, cl, pack, stars, priors, n_pops, 2, 2, rows)
    assert got_star.shape[1] == 2 + 3 * n_filt and got_rows.shape[1] == 1 + 6 * n_filt and (got_star[:, 1] > 0).sum() >= 40


# ---- 3 / 4. edges of the shapes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_wd", [0, 1, 4, 5])
@pytest.mark.parametrize("n_ms", [1, 64, 65])
def test_star_count_edges(n_ms, n_wd):
    pack_d, cl, pack, _, priors, _ = build_problem("parsec", 4, n_stars=400, wd_frac=0.1, seed=12)
    stage = np.asarray(cl["stage"])
    ms, wd = np.flatnonzero(stage != abi.STAGE_WD)[:n_ms], np.flatnonzero(stage == abi.STAGE_WD)[:n_wd]
    assert len(ms) == n_ms and len(wd) == n_wd
    cl = tm.subset(cl, np.sort(np.concatenate([ms, wd])))
    against_reference(pack_d, cl, pack, abi.make_stars(cl), priors, 1, 2, 2, tm.rows_for(pack_d, cl, 1, 2))


@pytest.mark.parametrize("n_eep,K,n_chunks", [(40, 1, 1), (90, 3, 5)])
def test_node_table_edges(n_eep, K, n_chunks):
    """One partial 64-node chunk; five chunks, the last one partial."""
    pack_d, cl, pack, stars, priors, _ = build_problem("parsec", 4, n_stars=70, wd_frac=0.1, seed=12, n_eep=n_eep)
    assert ((int(np.max(pack_d["iso_n_eep"])) - 1) * K + 63) // 64 == n_chunks
    against_reference(pack_d, cl, pack, stars, priors, 1, K, 2, tm.rows_for(pack_d, cl, 1))


# ---- 5. special stars -------------------------------------------------------------------------------------------------------
def test_special_stars():
    """A star with every filter unused, one with (all but) no membership prior, one with membership prior 1, and an MS/RGB and a
    WD-stage star with a single filter unused each: for that filter l_f == 0 exactly and the star is absent from the filter's
    N .. E -- shown on one row, where star_loo IS the increment, by re-adding N_f and E_f in the kernel's order."""
    pack_d, cl, pack, _, priors, _ = build_problem("parsec", 4, n_stars=70, wd_frac=0.1, seed=12)
    cl = tm.subset(cl, np.arange(70))
    cl["sigma"] = np.array(cl["sigma"], dtype=np.float64)
    cl["clust_prior"] = np.array(cl["clust_prior"], dtype=np.float64)
    ms = np.flatnonzero((np.asarray(cl["stage"]) != abi.STAGE_WD) & (cl["sigma"] > 0).all(axis=1))
    cl["sigma"][ms[3]] = -1.0
    cl["clust_prior"][ms[5]] = 1e-300
    cl["clust_prior"][ms[7]] = 1.0
    cl["sigma"][ms[9], 1] = -1.0
    wd = np.flatnonzero((np.asarray(cl["stage"]) == abi.STAGE_WD) & (cl["sigma"] > 0).all(axis=1))
    cl["sigma"][wd[0], 2] = -1.0
    rows = tm.rows_for(pack_d, cl, 1)
    stars = abi.make_stars(cl)
    got, got_rows, want, _ = against_reference(pack_d, cl, pack, stars, priors, 1, 2, 2, rows)
    assert want[wd[0], 1] > 0 and got[wd[0], 1] > 0
    assert got[ms[5], 0] == 3 and np.all(np.abs(got[ms[5], 1:]) < 1e-250)
    assert got[ms[7], 1] == 3.0
    assert got[ms[3], 0] == 3 and got[ms[3], 1] > 0 and np.all(got[ms[3], 3::3] > 0) and np.all(got[ms[3], 4::3] == 0)
    assert got[ms[9], 4 + 3 * 1] == 0 and got[wd[0], 4 + 3 * 2] == 0 and got[ms[9], 4 + 3 * 0] != 0 and got[wd[0], 4 + 3 * 0] != 0
    tab = lr.star_table(got, cl)
    assert 5 < tab[ms[9], 2 + 5 * 1] < 40 and tab[ms[9], 4 + 5 * 1] == 0 and 5 < tab[wd[0], 2 + 5 * 2] < 40 and tab[wd[0], 6 + 5 * 2] == 0
    eng = make_engine(pack, stars, priors, 1, 2, 2)
    try:
        x, rws = eng.filter_loo(rows[:1])
    finally:
        eng.close()
    for f in range(4):
        a = e = 0.0
        for i in range(70):
            if cl["sigma"][i, f] > 0:
                a = a + x[i, 1]
                e = e + x[i, 4 + 3 * f]
        assert rws[0, 1 + 6 * f] == a and rws[0, 6 + 6 * f] == e
    assert rws[0, 1 + 6 * 1] < rws[0, 1 + 6 * 0] and x[ms[9], 1] > 0


# ---- 6. promotion and the rescale path --------------------------------------------------------------------------------------
def test_rescale_path():
    """Photometry five times sharper: the largest term of most stars lies more than 600 e-folds above the seed, so every
    leave-out's reference must jump and its three sums be rescaled."""
    import numpy_ref
    pack_d, cl, pack, _, priors, _ = build_problem("parsec", 4, n_stars=70, wd_frac=0.1, seed=12)
    cl = tm.subset(cl, np.arange(70))
    sig = np.asarray(cl["sigma"], dtype=np.float64)
    cl["sigma"] = np.where(sig > 0, 0.2 * sig, sig)
    rows = tm.rows_for(pack_d, cl, 1, 2, outside=False)
    t, gm, _ = numpy_ref.marg_terms(pack_d, cl, rows[0], 2, 2, 0)
    n_primary = len(gm) // 2
    t = np.where(np.isfinite(t), t, -np.inf)
    ms = np.asarray(cl["stage"]) != abi.STAGE_WD
    jump = (t.max(axis=1) - t[:, 0:n_primary:16].max(axis=1))[ms]
    print(f"{(jump > 600).sum()} of {ms.sum()} stars jump by more than 600 e-folds above the seed; the largest jump {jump.max():.4g}")
    assert (jump > 600).sum() >= 40
    against_reference(pack_d, cl, pack, abi.make_stars(cl), priors, 1, 2, 2, rows)


@pytest.mark.parametrize("name,n_filt,n_y,n_pops", [("parsec", 4, 1, 1), ("dsed", 5, 3, 2)])
def test_promoted_pairs(name, n_filt, n_y, n_pops):
    """The non-vacuity fixtures with every membership prior 1, so that the outliers -- the pairs whose largest leave-out term
    lies thousands of e-folds above the largest full term -- carry their full weight: their leave-out prediction and density
    against the reference, pair by pair, besides the whole comparison."""
    pack_d, cl, pack, _, priors, _ = build_problem(name, n_filt, n_stars=70, wd_frac=0.1, n_y=n_y, n_pops=n_pops, seed=12)
    cl = tm.subset(cl, np.arange(70))
    cl["clust_prior"] = np.ones(70)
    row = tm.rows_for(pack_d, cl, n_pops)[:1]
    nodes = mr.star_nodes(pack_d, cl, row[0], n_pops, 2, 2)
    nv = lr.non_vacuity(pack_d, cl, row[0], n_pops, 2, 2, nodes)
    print(f"{nv['promoted']} promoted pairs, by up to {nv['max_promotion']:.6g} e-folds; {nv['revived']} nodes live only when left out")
    assert nv["promoted"] >= 3 and nv["max_promotion"] > 1e4 and nv["revived"] >= 100
    got, _, want, _ = against_reference(pack_d, cl, pack, abi.make_stars(cl), priors, n_pops, 2, 2, row, [nodes])
    for i, f in nv["promoted_pairs"]:
        assert want[i, 1] == 1.0 and got[i, 1] == 1.0
        assert abs(got[i, 2 + 3 * f] - want[i, 2 + 3 * f]) <= 1e-9 * max(1.0, abs(want[i, 2 + 3 * f]))
        assert abs(got[i, 4 + 3 * f] - want[i, 4 + 3 * f]) <= 1e-9 * max(1.0, abs(want[i, 4 + 3 * f])) and want[i, 4 + 3 * f] < -25


# ---- 7. the route the library had before ------------------------------------------------------------------------------------
def test_reload_route():
    """Every membership prior 1 (p = 1 exactly), one row at a time, for every filter f: the stars reloaded with sigma[:, f] = -1.
    b9_phot_resid's predicted magnitude in f then equals looMag within 1e-9 mag, and the marginalised per-star b9_logpost of the
    full catalogue minus the same with f disabled equals l_f within 1e-9 max(1, |operands|)."""
    pack_d, cl, pack, _, priors, _ = build_problem("parsec", 4, n_stars=70, wd_frac=0.1, seed=12)
    cl = tm.subset(cl, np.arange(70))
    cl["clust_prior"] = np.ones(70)
    cl["sigma"] = np.array(cl["sigma"], dtype=np.float64)
    obs = np.asarray(cl["obs"], dtype=np.float64)
    rows = tm.rows_for(pack_d, cl, 1, outside=False)
    eng = make_engine(pack, abi.make_stars(cl), priors, 1, 2, 2, abi.MODE_MARGINALISED)
    try:
        loo = [eng.filter_loo(r[None, :], want_rows=False)[0] for r in rows]
        full = [eng.logpost(r[None, :], perstar=True)[1][0] for r in rows]
        for f in range(4):
            cf = dict(cl)
            cf["sigma"] = cl["sigma"].copy()
            cf["sigma"][:, f] = -1.0
            eng.load_stars(abi.make_stars(cf))
            for k, r in enumerate(rows):
                resid = eng.phot_resid(r[None, :], want_rows=False)[0]
                less = eng.logpost(r[None, :], perstar=True)[1][0]
                used = cl["sigma"][:, f] > 0
                both = (loo[k][:, 1] > 0) & (resid[:, 1] > 0) & np.isfinite(full[k]) & np.isfinite(less) & used
                assert both.sum() >= 60
                assert np.all(loo[k][both, 1] == 1.0) and np.all(resid[both, 1] == 1.0)
                loo_mag, pred = obs[both, f] + loo[k][both, 2 + 3 * f], resid[both, 2 + 2 * f]
                lpd = loo[k][both, 4 + 3 * f]
                diff = full[k][both] - less[both]
                scale = np.maximum(1.0, np.maximum(np.abs(full[k][both]), np.abs(less[both])))
                print(f"filter {f} row {k}: {both.sum()} stars, largest |looMag - predMag| {np.abs(loo_mag - pred).max():.3g} mag, largest "
                      f"|l_f - (v - v^f)| / scale {(np.abs(lpd - diff) / scale).max():.3g}")
                assert np.all(np.abs(loo_mag - pred) <= 1e-9)
                assert np.all(np.abs(lpd - diff) <= 1e-9 * scale)
    finally:
        eng.close()


# ---- 8. ties ----------------------------------------------------------------------------------------------------------------
def test_ties_to_star_moments_and_phot_resid():
    """x[0] is b9_star_moments' ROWS; x[1] and the two sums of a filter the star does not use are b9_phot_resid's: bit for bit
    under marg_no_pruning, within rtol 1e-12 otherwise."""
    pack_d, cl, pack, _, priors, rows, _, _ = case(0)
    cl = tm.subset(cl, np.arange(len(cl["mass1"])))
    cl["sigma"] = np.array(cl["sigma"], dtype=np.float64)
    cl["sigma"][::4, 1] = -1.0
    cl["sigma"][1::8, 4] = -1.0
    unused = ~(cl["sigma"] > 0)
    eng = make_engine(pack, abi.make_stars(cl), priors, 2, 2, 2)
    try:
        mom = eng.star_moments(rows)
        res, _ = eng.phot_resid(rows)
        loo, _ = eng.filter_loo(rows)
        eng.set_tuning(marg_no_pruning=1)
        res_full, _ = eng.phot_resid(rows)
        loo_full, _ = eng.filter_loo(rows)
    finally:
        eng.close()
    assert np.array_equal(loo[:, 0], mom[:, abi.MOM_ROWS]) and (loo[:, 0] == 3).sum() >= 100
    live = loo[:, 1] > 0
    sel = unused & live[:, None]
    assert sel.sum() >= 30 and (sel.any(axis=0)).sum() >= 2
    assert np.array_equal(loo_full[:, 1], res_full[:, 1])
    assert np.array_equal(loo_full[:, 2::3][sel], res_full[:, 2::2][sel]) and np.array_equal(loo_full[:, 3::3][sel], res_full[:, 3::2][sel])
    np.testing.assert_allclose(loo[:, 1], res[:, 1], rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(loo[:, 2::3][sel], res[:, 2::2][sel], rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(loo[:, 3::3][sel], res[:, 3::2][sel], rtol=1e-12, atol=1e-300)
    assert np.all(loo[:, 4::3][unused] == 0) and np.all(loo_full[:, 4::3][unused] == 0)


# ---- 9. bitwise invariances -------------------------------------------------------------------------------------------------
def test_bitwise_invariances():
    pack_d, cl, pack, stars, priors, _, _, _ = case(0)
    rows = synth.walker_params(cl["truth"], 40, seed=8, scale=0.3, n_pops=2)
    outside = rows[0].copy(); outside[abi.P_LOGAGE] = pack_d["log_age"][-1] + 1.0
    edges = np.linspace(0.1, 8.0, 25)
    eng = make_engine(pack, stars, priors, 2, 2, 2)
    try:
        whole, whole_rows = eng.filter_loo(rows)
        assert (whole[:, 0] == 40).sum() >= 120
        # 40 rows in one call (two chunks) = the same rows as 1 + 32 + 7 continued = chunked by hand into 8s
        acc, r0 = eng.filter_loo(rows[:1])
        acc, r1 = eng.filter_loo(rows[1:33], acc)
        acc, r2 = eng.filter_loo(rows[33:], acc)
        assert np.array_equal(acc, whole) and np.array_equal(np.concatenate([r0, r1, r2]), whole_rows)
        acc = None
        for r in range(0, 40, 8):
            acc, rws = eng.filter_loo(rows[r:r + 8], acc)
            assert np.array_equal(rws, whole_rows[r:r + 8])
        assert np.array_equal(acc, whole)
        # a row alone = the same row in slot 35 of a batch of rows outside the grid
        j = 17
        alone, alone_row = eng.filter_loo(rows[j:j + 1])
        assert np.array_equal(alone_row[0], whole_rows[j])
        batch = np.tile(outside, (36, 1)); batch[35] = rows[j]
        got, got_rows = eng.filter_loo(batch, np.zeros_like(alone))
        assert np.array_equal(got_rows[35], whole_rows[j]) and np.all(got_rows[:35] == 0) and np.array_equal(got, alone)
        # star_loo is the same whether row_loo is NULL or not, and the other way round
        only_star, none = eng.filter_loo(rows, want_rows=False)
        assert none is None and np.array_equal(only_star, whole)
        none, only_rows = eng.filter_loo(rows, want_star=False)
        assert none is None and np.array_equal(only_rows, whole_rows)
        # a repeated call; b9_mass_hist, b9_star_moments and b9_phot_resid calls in between leave nothing behind
        eng.mass_hist(rows[:5], edges, abi.HQ_SYSTEM)
        eng.star_moments(rows[:7])
        eng.phot_resid(rows[:3])
        again, again_rows = eng.filter_loo(rows)
        assert np.array_equal(again, whole) and np.array_equal(again_rows, whole_rows)
    finally:
        eng.close()
    eng = make_engine(pack, stars, priors, 2, 2, 2)                           # a fresh context
    try:
        fresh, fresh_rows = eng.filter_loo(rows)
        assert np.array_equal(fresh, whole) and np.array_equal(fresh_rows, whole_rows)
    finally:
        eng.close()
    # a star's line does not depend on the other stars of the catalogue: every third star alone (other lane-mates, other chunks)
    keep = np.arange(0, len(cl["mass1"]), 3)
    eng = make_engine(pack, abi.make_stars(tm.subset(cl, keep)), priors, 2, 2, 2)
    try:
        part, _ = eng.filter_loo(rows)
    finally:
        eng.close()
    assert np.array_equal(part, whole[keep]) and (part[:, 1] > 0).sum() >= 30


# ---- 10. the scratch rule ---------------------------------------------------------------------------------------------------
def test_scratch_rule_picks_the_chunk():
    """16 filters, 6000 stars: a row's increments take 8 x 6000 x 50 B = 2.4 MB, so the 64 MiB rule allows 27 rows a chunk -- below
    the 32-row cap.  30 rows in one call (27 + 3) = 15 + 15 continued."""
    pack_d, cl, pack, stars, priors, _ = build_problem("parsec", 16, n_stars=6000, wd_frac=0.02, seed=12)
    assert (64 << 20) // (8 * 6000 * 50) == 27
    rows = synth.walker_params(cl["truth"], 30, seed=8, scale=0.3)
    eng = make_engine(pack, stars, priors, 1, 1, 2)
    try:
        whole, whole_rows = eng.filter_loo(rows)
        acc, r0 = eng.filter_loo(rows[:15])
        acc, r1 = eng.filter_loo(rows[15:], acc)
    finally:
        eng.close()
    assert (whole[:, 0] == 30).sum() >= 5000
    assert np.array_equal(acc, whole) and np.array_equal(np.concatenate([r0, r1]), whole_rows)


# ---- 11. leaves the sampler alone -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [abi.MODE_GIVEN_MASS, abi.MODE_MARGINALISED])
def test_sampler_blocks_are_untouched(mode):
    from base_amd import mcmc
    pack_d, cl, pack, stars, priors, _, _, _ = case(1)
    free = np.array(mcmc.DEFAULT_FREE)
    chol = np.diag([mcmc.DEFAULT_STEP[k] for k in free]) * 0.3
    start = synth.walker_params(cl["truth"], 4, seed=2, scale=0.3)
    rows = tm.rows_for(pack_d, cl, 1)

    def run(interleave):
        eng = make_engine(pack, stars, priors, 1, 1, 4, mode)
        try:
            lp0 = eng.logpost(start)
            h = eng.mcmc_submit(start, lp0, np.arange(4), free, chol, 11, 0, 6, asynchronous=True)
            if interleave:
                with pytest.raises(Exception) as e:                        # B9_ERR_STATE: a block is outstanding
                    eng.filter_loo(rows)
                assert e.value.code == abi.B9_ERR_STATE and "outstanding" in str(e.value)
            first = [np.array(x) for x in eng.mcmc_collect(h)[:4]]
            if interleave:
                star, _ = eng.filter_loo(rows)
                assert (star[:, 0] == 3).sum() >= 100
            h = eng.mcmc_submit(start, lp0, np.arange(4), free, chol, 11, 6, 6, cont=True, asynchronous=True)
            second = [np.array(x) for x in eng.mcmc_collect(h)[:4]]
        finally:
            eng.close()
        return first + second

    for a, b in zip(run(False), run(True)):
        assert np.array_equal(a, b)


# ---- 12. errors -------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_untouched():
    from base_amd import mcmc
    pack_d, cl, pack, stars, priors, rows = small()
    eng = make_engine(pack, stars, priors, 1, 2, 2)
    try:
        n = eng.n_stars
        rows = np.ascontiguousarray(rows)

        def call(n_rows=4, star=True, rws=True, params=True, ctx=True):
            sl, rl = np.full((n, 14), 7.25), np.full((4, 25), 7.25)
            code = eng.lib.b9_filter_loo(eng._ctx if ctx else None, rows.ctypes.data_as(_dp) if params else None, n_rows, 0,
                                         sl.ctypes.data_as(_dp) if star else None, rl.ctypes.data_as(_dp) if rws else None)
            assert code == abi.B9_OK or (np.all(sl == 7.25) and np.all(rl == 7.25))
            return code

        assert call() == abi.B9_OK
        assert call(n_rows=0) == abi.B9_ERR_INVALID and call(n_rows=-2) == abi.B9_ERR_INVALID
        assert call(star=False, rws=False) == abi.B9_ERR_INVALID
        assert call(params=False) == abi.B9_ERR_INVALID
        assert call(ctx=False) == abi.B9_ERR_INVALID
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


# ---- 13. the CLI ------------------------------------------------------------------------------------------------------------
def test_cli_filter_check(tmp_path):
    """simCluster (200 stars) -> scatterCluster -> singlePopMcmc (short, 4 walkers x 100 main-run rows: the program passes them
    in two batches, the second continued) -> filterCheck --perStar: both files read back to the bits of what Engine.filter_loo
    in ONE call gives through hostlib.loo_table / filter_loo_table.  The chain sits on the truth the catalogue was drawn from:
    every band's mean predictive z^2 over the members lies in (0.2, 5)."""
    from base_amd import build, engine, host_build, hostlib
    from cli_util import cli as _cli
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
    r = _cli("filterCheck", "--config", y, "--perStar")
    assert r.returncode == 0, r.stderr
    assert "star rows/s" in r.stderr

    cl = tm._read_phot(base + ".sim.scatter")
    header = open(base + ".sim.scatter").read().splitlines()[0].split()
    filters = header[1:1 + cl["n_filt"]]
    phot_ids = [ln.split()[0] for ln in open(base + ".sim.scatter").read().splitlines()[1:]]
    rows = hostlib.read_res_rows(fit + ".res", start, 3)
    assert len(rows) == 100 * 4                           # more than one batch of 256
    obs, sigma = cl["obs"].reshape(-1, cl["n_filt"]), cl["sigma"].reshape(-1, cl["n_filt"])
    eng = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cl), synth.default_priors(pack_d, truth), tm.opts(1, K, Q))
    try:
        star, rws = eng.filter_loo(rows)
    finally:
        eng.close()
    ids, cols, tab = hostlib.read_star_filter_check(fit + ".starFilterCheck")
    assert ids == phot_ids and cols == ["rows", "member"] + [f"{f}_{c}" for f in filters for c in hostlib.LOO_STAR_COLUMNS]
    assert np.array_equal(tab, hostlib.loo_table(star, obs, sigma))
    assert np.all(tab[:, 0] == len(rows)) and (tab[:, 1] > 0.9).sum() >= 100
    names, cols, ftab = hostlib.read_filter_check(fit + ".filterCheck")
    assert names == filters and cols == list(hostlib.FILTER_CHECK_COLUMNS)
    assert np.array_equal(ftab, hostlib.filter_loo_table(rws, cl["n_filt"]))
    members = tab[:, 1] > 0.9
    z2 = np.array([np.mean(tab[members & (sigma[:, f] > 0), 5 + 5 * f] ** 2) for f in range(cl["n_filt"])])
    print(f"mean predictive z^2 per band over {members.sum()} members: {np.round(z2, 3)}")
    assert np.all(ftab[:, 0] == len(rows)) and np.all(z2 > 0.2) and np.all(z2 < 5)
