"""b9_phot_resid (the photResiduals counterpart) on the GPU: star_resid and row_resid against the numpy statement
tests/resid_ref.py, the edges of the star, node and filter shapes, the rescale path, bit-for-bit invariances, the sampler left
alone, the ties to b9_star_moments, b9_predict_mags and b9_sample_mass, the errors, and the CLI.  Each test makes its own
short-lived engine on the small packs of build_problem(small=True); a case's reference nodes are computed once and shared.

Tolerances: tests/resid_check.py (rtol 1e-9 + the pruning's bound per column + the cancellation term of the first moments;
with b9_tuning.marg_no_pruning the pruning's bound is dropped)."""
import ctypes as C
import functools

import numpy as np
import pytest

import moments_ref as mr
import resid_check as rc
import resid_ref as rr
import test_gpu_moments as tm
from base_amd import abi, synth
from conftest import build_problem
from cli_util import cli as _cli

pytestmark = pytest.mark.gpu
_dp = C.POINTER(C.c_double)


def make_engine(pack, stars, priors, n_pops, K, Q, mode=abi.MODE_GIVEN_MASS):
    from base_amd import engine
    return engine.Engine(pack, stars, priors, tm.opts(n_pops, K, Q, mode))


def against_reference(pack_d, cl, pack, stars, priors, n_pops, K, Q, rows, nodes=None, n_nodes=None, ref=None):
    """Both outputs, with the pruning and without it, against the reference; returns (got_star, got_rows, want_star, want_rows)."""
    n_nodes = n_nodes or tm.n_nodes_of(pack_d, n_pops, K, Q)
    want_star, want_rows, x, bound, absx = ref or rr.reference(pack_d, cl, rows, n_pops, K, Q, nodes)
    eng = make_engine(pack, stars, priors, n_pops, K, Q)
    try:
        got_star, got_rows = eng.phot_resid(rows)
        eng.set_tuning(marg_no_pruning=1)
        full_star, full_rows = eng.phot_resid(rows)
        eng.set_tuning()
    finally:
        eng.close()
    print(f"largest relative difference among the entries above 1e-6: star_resid {rc.largest_rel(got_star, want_star):.3g} "
          f"(unpruned {rc.largest_rel(full_star, want_star):.3g}), row_resid {rc.largest_rel(got_rows, want_rows):.3g} "
          f"(unpruned {rc.largest_rel(full_rows, want_rows):.3g})")
    sig = cl["sigma"]
    rc.assert_star_resid(got_star, want_star, rc.star_atol(bound, absx, n_nodes))
    rc.assert_row_resid(got_rows, want_rows, rc.row_atol(bound, absx, sig, n_nodes))
    rc.assert_variances(got_star, want_star, cl)
    rc.assert_star_resid(full_star, want_star, rc.star_atol(bound, absx, n_nodes, pruning=False))
    rc.assert_row_resid(full_rows, want_rows, rc.row_atol(bound, absx, sig, n_nodes, pruning=False))
    rc.assert_variances(full_star, want_star, cl)
    return got_star, got_rows, want_star, want_rows


@functools.lru_cache(maxsize=None)
def case(k):
    """Case k of test_gpu_moments.CASES with its rows (3 + one outside the grid) and the reference, built once."""
    name, n_filt, n_y, n_pops, K, Q, n_stars, wd_frac, n_nodes = tm.CASES[k]
    pack_d, cl, pack, stars, priors, _ = build_problem(name, n_filt, n_stars=n_stars, wd_frac=wd_frac, n_y=n_y, n_pops=n_pops, seed=12)
    rows = tm.rows_for(pack_d, cl, n_pops)
    rows.setflags(write=False)
    nodes = rr.nodes_of_rows(pack_d, cl, rows, n_pops, K, Q)
    return pack_d, cl, pack, stars, priors, rows, nodes, rr.reference(pack_d, cl, rows, n_pops, K, Q, nodes)


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
    """Figures of the reference (live stars, with predSd > 1e-6 in some filter, stars with an unused filter, live WD-stage
    stars): dsed 5: 127 127 7 11; parsec 8: 123 123 13 11; girardi 3: 69 69 3 0; parsec 9: 67 63 1 6."""
    name, n_filt, n_y, n_pops, K, Q, n_stars, wd_frac, n_nodes = tm.CASES[k]
    pack_d, cl, pack, stars, priors, rows, nodes, ref = case(k)
    # not vacuous: stated on the reference before the device is consulted
    live, spread, unused, wd = rc.non_vacuity(ref[0], cl)
    print(f"{name} {n_filt}: {live} live, {spread} with predSd > 1e-6, {unused} with an unused filter, {wd} live WD-stage stars")
    assert unused >= 1 and spread >= (live * 9) // 10
    if k == 0:
        assert live >= 90 and spread == live
    if wd_frac > 0:
        assert wd >= 1
    got_star, got_rows, want_star, want_rows = against_reference(pack_d, cl, pack, stars, priors, n_pops, K, Q, rows, nodes, n_nodes, ref)
    assert np.all(got_rows[-1] == 0) and np.all(got_star[got_star[:, 0] > 0, 0] == 3)      # the row outside the grid adds nothing
    assert got_star.shape == (n_stars, 2 + 2 * n_filt) and got_rows.shape == (4, 1 + 5 * n_filt)


# ---- 2. edges of the shapes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_wd", [0, 1, 4, 5])
@pytest.mark.parametrize("n_ms", [1, 64, 65])
def test_star_count_edges(n_ms, n_wd):
    pack_d, cl, pack, _, priors, _ = build_problem("parsec", 4, n_stars=400, wd_frac=0.1, seed=12)
    stage = np.asarray(cl["stage"])
    ms, wd = np.flatnonzero(stage != abi.STAGE_WD)[:n_ms], np.flatnonzero(stage == abi.STAGE_WD)[:n_wd]
    assert len(ms) == n_ms and len(wd) == n_wd
    cl = tm.subset(cl, np.sort(np.concatenate([ms, wd])))
    against_reference(pack_d, cl, pack, abi.make_stars(cl), priors, 1, 2, 2, tm.rows_for(pack_d, cl, 1, 2))


@pytest.mark.parametrize("n_pops", [1, 2])
@pytest.mark.parametrize("n_filt", [4, 5, 8, 9, 16])
def test_every_instance(n_filt, n_pops):
    """The six instances, and 5 and 9 filters: padded rows on both sides of the 8 | 16 seam (filters are not tiled: there is
    no other seam).  The outputs hold n_filt filters only, so a padded filter has no column to leak into; that it does not
    disturb the real ones is the comparison itself."""
    pack_d, cl, pack, stars, priors, _ = build_problem("dsed", n_filt, n_stars=70, wd_frac=0.1, n_y=3 if n_pops == 2 else 1, n_pops=n_pops, seed=12)
    rows = tm.rows_for(pack_d, cl, n_pops, 2, outside=False)
    got_star, got_rows, _, _ = against_reference(pack_d, cl, pack, stars, priors, n_pops, 2, 2, rows)
    assert got_star.shape[1] == 2 + 2 * n_filt and got_rows.shape[1] == 1 + 5 * n_filt and (got_star[:, 1] > 0).sum() >= 50


@pytest.mark.parametrize("n_eep,K,n_chunks", [(40, 1, 1), (90, 3, 5)])
def test_node_table_edges(n_eep, K, n_chunks):
    """One partial 64-node chunk; five chunks, the last one partial."""
    pack_d, cl, pack, stars, priors, _ = build_problem("parsec", 4, n_stars=70, wd_frac=0.1, seed=12, n_eep=n_eep)
    assert ((int(np.max(pack_d["iso_n_eep"])) - 1) * K + 63) // 64 == n_chunks
    against_reference(pack_d, cl, pack, stars, priors, 1, K, 2, tm.rows_for(pack_d, cl, 1))


def test_special_stars():
    """A star with every filter unused (weighted by the prior over the grid), one with (all but) no membership prior
    (b9_load_stars refuses 0: tests/test_gpu_moments.py), one with membership prior 1, and an MS/RGB and a WD-stage star with
    a single filter unused each: the two sums in that filter are the reference's prediction, and it is absent from that filter's N .. D -- shown on one
    row, where star_resid IS the increment, by re-adding N_f in the kernel's order."""
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
    cl["sigma"][wd[0], 2] = -1.0                          # ... and a WD-stage star with one: its pivot there is 0 as well
    rows = tm.rows_for(pack_d, cl, 1)
    stars = abi.make_stars(cl)
    got, got_rows, want, _ = against_reference(pack_d, cl, pack, stars, priors, 1, 2, 2, rows)
    assert want[wd[0], 1] > 0 and got[wd[0], 1] > 0      # (a live member in the reference, so the comparison above covers it)
    assert got[ms[5], 0] == 3 and np.all(np.abs(got[ms[5], 1:]) < 1e-250)
    assert got[ms[7], 1] == 3.0
    assert got[ms[3], 0] == 3 and got[ms[3], 1] > 0 and np.all(got[ms[3], 3::2] > 0)
    tab = rr.star_table(got, cl)
    assert np.all(tab[ms[3], 3::4] > 0.5)                                  # no photometry: the prior's spread over the grid, in magnitudes
    assert 5 < tab[ms[9], 2 + 4 * 1] < 40 and tab[ms[9], 4 + 4 * 1] == 0   # a predicted magnitude in the band it lacks, no residual
    assert 5 < tab[wd[0], 2 + 4 * 2] < 40 and tab[wd[0], 4 + 4 * 2] == 0 and tab[wd[0], 5 + 4 * 2] == 0
    eng = make_engine(pack, stars, priors, 1, 2, 2)
    try:
        x, rws = eng.phot_resid(rows[:1])
    finally:
        eng.close()
    for f in range(4):
        a = 0.0
        for i in range(70):
            if cl["sigma"][i, f] > 0:
                a = a + x[i, 1]
        assert rws[0, 1 + 5 * f] == a
    assert rws[0, 1 + 5 * 1] < rws[0, 1 + 5 * 0] and x[ms[9], 1] > 0


def test_rescale_path():
    """Photometry five times sharper: the largest term of most stars lies more than 600 e-folds above the seed (the best of
    every 16th node at mass ratio 0), so the online reference must jump and every weighted sum be rescaled."""
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
    against_reference(pack_d, cl, pack, abi.make_stars(cl), priors, 1, 2, 2, rows)


# ---- 3. bitwise invariances -------------------------------------------------------------------------------------------------
def test_bitwise_invariances():
    pack_d, cl, pack, stars, priors, _, _, _ = case(0)
    rows = synth.walker_params(cl["truth"], 40, seed=8, scale=0.3, n_pops=2)
    outside = rows[0].copy(); outside[abi.P_LOGAGE] = pack_d["log_age"][-1] + 1.0
    edges = np.linspace(0.1, 8.0, 25)
    eng = make_engine(pack, stars, priors, 2, 2, 2)
    try:
        whole, whole_rows = eng.phot_resid(rows)
        assert (whole[:, 0] == 40).sum() >= 120
        # 40 rows in one call (two chunks) = the same rows as 1 + 32 + 7 continued = chunked by hand into 8s
        acc, r0 = eng.phot_resid(rows[:1])
        acc, r1 = eng.phot_resid(rows[1:33], acc)
        acc, r2 = eng.phot_resid(rows[33:], acc)
        assert np.array_equal(acc, whole) and np.array_equal(np.concatenate([r0, r1, r2]), whole_rows)
        acc = None
        for r in range(0, 40, 8):
            acc, rws = eng.phot_resid(rows[r:r + 8], acc)
            assert np.array_equal(rws, whole_rows[r:r + 8])
        assert np.array_equal(acc, whole)
        # a row alone = the same row in slot 35 of a batch of rows outside the grid
        j = 17
        alone, alone_row = eng.phot_resid(rows[j:j + 1])
        assert np.array_equal(alone_row[0], whole_rows[j])
        batch = np.tile(outside, (36, 1)); batch[35] = rows[j]
        got, got_rows = eng.phot_resid(batch, np.zeros_like(alone))
        assert np.array_equal(got_rows[35], whole_rows[j]) and np.all(got_rows[:35] == 0) and np.array_equal(got, alone)
        # star_resid is the same whether row_resid is NULL or not, and the other way round
        only_star, none = eng.phot_resid(rows, want_rows=False)
        assert none is None and np.array_equal(only_star, whole)
        none, only_rows = eng.phot_resid(rows, want_star=False)
        assert none is None and np.array_equal(only_rows, whole_rows)
        # a repeated call; a b9_mass_hist and a b9_star_moments call in between leave nothing behind
        eng.mass_hist(rows[:5], edges, abi.HQ_SYSTEM)
        eng.star_moments(rows[:7])
        again, again_rows = eng.phot_resid(rows)
        assert np.array_equal(again, whole) and np.array_equal(again_rows, whole_rows)
    finally:
        eng.close()
    eng = make_engine(pack, stars, priors, 2, 2, 2)                           # a fresh context
    try:
        fresh, fresh_rows = eng.phot_resid(rows)
        assert np.array_equal(fresh, whole) and np.array_equal(fresh_rows, whole_rows)
    finally:
        eng.close()


def test_scratch_rule_picks_the_chunk():
    """16 filters, 8000 stars: a row's increments take 8 x 8000 x 34 B = 2.2 MB, so the 64 MiB rule allows 30 rows a chunk --
    below the 32-row cap.  33 rows in one call (30 + 3) = 16 + 17 continued (chunks of 16 and 17, under both limits)."""
    pack_d, cl, pack, stars, priors, _ = build_problem("parsec", 16, n_stars=8000, wd_frac=0.02, seed=12)
    assert (64 << 20) // (8 * 8000 * 34) == 30
    rows = synth.walker_params(cl["truth"], 33, seed=8, scale=0.3)
    eng = make_engine(pack, stars, priors, 1, 1, 2)
    try:
        whole, whole_rows = eng.phot_resid(rows)
        acc, r0 = eng.phot_resid(rows[:16])
        acc, r1 = eng.phot_resid(rows[16:], acc)
    finally:
        eng.close()
    assert (whole[:, 0] == 33).sum() >= 7000
    assert np.array_equal(acc, whole) and np.array_equal(np.concatenate([r0, r1]), whole_rows)


# ---- 4. leaves the sampler alone --------------------------------------------------------------------------------------------
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
                    eng.phot_resid(rows)
                assert e.value.code == abi.B9_ERR_STATE and "outstanding" in str(e.value)
            first = [np.array(x) for x in eng.mcmc_collect(h)[:4]]
            if interleave:
                star, _ = eng.phot_resid(rows)
                assert (star[:, 0] == 3).sum() >= 100
            h = eng.mcmc_submit(start, lp0, np.arange(4), free, chol, 11, 6, 6, cont=True, asynchronous=True)
            second = [np.array(x) for x in eng.mcmc_collect(h)[:4]]
        finally:
            eng.close()
        return first + second

    for a, b in zip(run(False), run(True)):
        assert np.array_equal(a, b)


# ---- 5. ties to existing calls, on the device -------------------------------------------------------------------------------
def test_ties_to_star_moments():
    pack_d, cl, pack, stars, priors, rows, _, _ = case(0)
    eng = make_engine(pack, stars, priors, 2, 2, 2)
    try:
        mom = eng.star_moments(rows)
        star, rws = eng.phot_resid(rows)
    finally:
        eng.close()
    assert np.array_equal(star[:, 0], mom[:, abi.MOM_ROWS]) and (star[:, 0] == 3).sum() >= 100
    np.testing.assert_allclose(star[:, 1], mom[:, abi.MOM_MEMBER], rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(rws[:, 0].sum(), mom[:, abi.MOM_MEMBER].sum(), rtol=1e-12)


def test_sharpened_star_predicts_its_node():
    """A star whose observations are b9_predict_mags at a grid node (as b9_sample_mass reports it), sigma 50 x sharper: predMag
    is that node's magnitudes within 1e-9, predSd ~ 0.  The reference says the same of this catalogue before the device is asked."""
    pack_d, cl, pack, stars, priors, _ = build_problem("parsec", 4, n_stars=20, wd_frac=0.0, seed=12)
    cl = dict(cl)
    par = np.array(cl["truth"], dtype=np.float64)
    i = 3
    eng = make_engine(pack, stars, priors, 1, 2, 2)
    try:
        mass, ratio, member, pop = eng.sample_mass(par[None, :], seed=5)
        assert mass[0, i] > 0
        mags, _ = eng.predict_mags(par, mass[0, i:i + 1], ratio[0, i:i + 1])
    finally:
        eng.close()
    cl["obs"] = np.array(cl["obs"], dtype=np.float64); cl["sigma"] = np.array(cl["sigma"], dtype=np.float64)
    cl["obs"][i] = mags[0]
    cl["sigma"][i] = np.abs(cl["sigma"][i]) / 50.0
    want = rr.star_table(rr.increments(pack_d, cl, par, 1, 2, 2)[0], cl)
    np.testing.assert_allclose(want[i, 2::4], mags[0], rtol=0, atol=1e-9)
    eng = make_engine(pack, abi.make_stars(cl), priors, 1, 2, 2)
    try:
        star, _ = eng.phot_resid(par[None, :])
    finally:
        eng.close()
    tab = rr.star_table(star, cl)
    np.testing.assert_allclose(tab[i, 2::4], mags[0], rtol=0, atol=1e-9)
    assert np.all(tab[i, 3::4] < 1e-4) and star[i, 1] > 0


Z_MAX = 6.0
SKEW_GUARD = 0.3


def draws_reference(pack_d, cl, rows, K, Q, R):
    """From the reference alone, two populations: (P [star] = sum_r p_r, p_r [row, star], the rows' mean magnitudes
    [row, star, nf], the variance of the member-weighted mean of R draws per row [star, nf], the guarded stars [star])."""
    n, nf = len(cl["mass1"]), pack_d["n_filt"]
    n_rows = len(rows)
    p_ref, mean_ref, var_ref, m3_ref = np.zeros((n_rows, n)), np.zeros((n_rows, n, nf)), np.zeros((n_rows, n, nf)), np.zeros((n_rows, n, nf))
    for r, par in enumerate(rows):
        nodes = mr.star_nodes(pack_d, cl, par, 2, K, Q)
        mags = rr.node_mags(pack_d, cl, par, nodes)
        for i in range(n):
            if mags[i] is None:
                continue
            w, L = mr.weights(nodes[i])
            p_ref[r, i] = mr.membership(cl, i, L)
            mean_ref[r, i] = (w[:, None] * mags[i]).sum(axis=0)
            dev = mags[i] - mean_ref[r, i]
            var_ref[r, i] = (w[:, None] * dev ** 2).sum(axis=0)
            m3_ref[r, i] = (w[:, None] * dev ** 3).sum(axis=0)
    P = p_ref.sum(axis=0)
    ok = P > 0
    pw = p_ref[:, :, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = (pw * mean_ref).sum(axis=0) / P[:, None]
        sh = mean_ref - mu[None]
        pooled_var = (pw * (var_ref + sh ** 2)).sum(axis=0) / P[:, None]
        pooled_m3 = (pw * (m3_ref + 3 * var_ref * sh + sh ** 3)).sum(axis=0) / P[:, None]
        gamma1 = pooled_m3 / pooled_var ** 1.5
        est_var = (pw ** 2 * var_ref).sum(axis=0) / (R * P[:, None] ** 2)
        guarded = ok & np.all(est_var > 0, axis=1) & np.all(np.abs(gamma1) / np.sqrt(n_rows * R) <= SKEW_GUARD, axis=1) & (p_ref > 0).all(axis=0)
    return P, p_ref, mean_ref, est_var, guarded


def test_statistics_against_device_draws():
    """Case 1, 40 rows drawn 10 times each (distinct row0): b9_sample_mass's nodes fed to b9_predict_mags row by row.  Per
    star and filter the member-weighted mean drawn magnitude sum p_r mag / sum p_r estimates predMag with variance
    sum_r p_r^2 Var_r / (R (sum_r p_r)^2) (R draws per row; p_r, Var_r: the reference's): |z| <= 6.  A star is tested when, in
    every filter, that variance is positive and the pooled skewness keeps |gamma_1| / sqrt(400) <= 0.3 (moments_ref.mass_z's
    guard).  The reference read without its pivot fails the same check."""
    name, n_filt, n_y, n_pops, K, Q, n_stars, wd_frac, n_nodes = tm.CASES[0]
    pack_d, cl, pack, stars, priors, _, _, _ = case(0)
    R = 10
    rows = synth.walker_params(cl["truth"], 40, seed=8, scale=0.3, n_pops=2)
    rows[:, abi.P_LAMBDA] = np.clip(rows[:, abi.P_LAMBDA], 0.05, 0.95)
    P, p_ref, mean_ref, est_var, guarded = draws_reference(pack_d, cl, rows, K, Q, R)
    n, nf = n_stars, n_filt
    print(f"{guarded.sum()} guarded stars of {n}")
    assert guarded.sum() >= 60

    eng = make_engine(pack, stars, priors, 2, K, Q)
    try:
        star, _ = eng.phot_resid(rows)
        num, den = np.zeros((n, nf)), np.zeros(n)
        for k in range(R):
            mass, ratio, member, pop = eng.sample_mass(rows, seed=20240611, row0=40 * k)
            for r in range(40):
                mags, _ = eng.predict_mags(rows[r], mass[r], ratio[r], wd_type=cl["wd_type"], pop=pop[r])
                live = mass[r] > 0
                num[live] += member[r, live, None] * mags[live]
                den[live] += member[r, live]
    finally:
        eng.close()
    drawn = num[guarded] / den[guarded, None]
    sd = np.sqrt(est_var[guarded])
    z = (drawn - rr.star_table(star, cl)[guarded, 2::4]) / sd
    print(f"largest |z| {np.abs(z).max():.3g}")
    assert np.abs(z).max() <= Z_MAX
    mutant = np.zeros_like(star)                         # the accumulators formed without the pivot: p sum w pred
    mutant[:, 0], mutant[:, 1], mutant[:, 2::2] = 40, P, (p_ref[:, :, None] * mean_ref).sum(axis=0)
    z_mut = (drawn - rr.star_table(mutant, cl)[guarded, 2::4]) / sd
    assert np.abs(z_mut).max() > 100 * Z_MAX


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_untouched():
    from base_amd import mcmc
    pack_d, cl, pack, stars, priors, rows = small()
    eng = make_engine(pack, stars, priors, 1, 2, 2)
    try:
        n = eng.n_stars
        rows = np.ascontiguousarray(rows)

        def call(n_rows=4, star=True, rws=True, params=True, ctx=True):
            sr, rr_ = np.full((n, 10), 7.25), np.full((4, 21), 7.25)
            code = eng.lib.b9_phot_resid(eng._ctx if ctx else None, rows.ctypes.data_as(_dp) if params else None, n_rows, 0,
                                         sr.ctypes.data_as(_dp) if star else None, rr_.ctypes.data_as(_dp) if rws else None)
            assert code == abi.B9_OK or (np.all(sr == 7.25) and np.all(rr_ == 7.25))
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


# ---- 7. the CLI ---------------------------------------------------------------------------------------------------------------
def test_cli_phot_residuals(tmp_path):
    """simCluster (200 stars) -> scatterCluster -> singlePopMcmc (short, 4 walkers x 100 main-run rows: the program passes
    them in two batches, the second continued) -> photResiduals --perStar: both files read back to the bits of what
    Engine.phot_resid in ONE call gives through hostlib.resid_table / filter_resid_table."""
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
    r = _cli("photResiduals", "--config", y, "--perStar")
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
        star, rws = eng.phot_resid(rows)
    finally:
        eng.close()
    ids, cols, tab = hostlib.read_phot_resid(fit + ".photResid")
    assert ids == phot_ids and cols == ["rows", "member"] + [f"{f}_{c}" for f in filters for c in hostlib.RESID_STAR_COLUMNS]
    assert np.array_equal(tab, hostlib.resid_table(star, obs, sigma))
    assert np.all(tab[:, 0] == len(rows)) and (tab[:, 1] > 0.9).sum() >= 100
    names, cols, ftab = hostlib.read_filter_resid(fit + ".filterResid")
    assert names == filters and cols == list(hostlib.FILTER_RESID_COLUMNS)
    assert np.array_equal(ftab, hostlib.filter_resid_table(rws, cl["n_filt"]))
    # the chain sits on the truth the catalogue was drawn from: every band's reduced chi^2 is of order one, its offset small
    assert np.all(ftab[:, 0] == len(rows)) and np.all(ftab[:, 1 + 5] > 0.2) and np.all(ftab[:, 1 + 5] < 5) and np.all(np.abs(ftab[:, 1 + 10]) < 0.05)
