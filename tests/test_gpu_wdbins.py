"""b9_wd_bins (the wdIntervals counterpart) on the GPU: the accumulators on every line's own edges against the numpy statement
tests/wdbins_ref.py (through the comparator and the edges of tests/wdbins_check.py), every kernel instance, the bin seams on the
device's own bits, the ties to b9_wd_moments and b9_star_bins, the bit-for-bit invariances, lines that add nothing, the errors,
sampler blocks left alone, and wd_intervals end to end with the wdIntervals program.  Each test makes its own short-lived engine.

Tolerance of every comparison with the reference: rtol 1e-9 per column plus 1e-9 of the line's total (wdbins_check.assert_close).
A line's edges for parity are its own: midpoints of the widest gaps between node values near the 31 levels k / 32 of its pooled
CDF, at least 10 tolerances of a node value away from every node of the line (the device's derived values agree with numpy's to
test_gpu_wdmass.check_derived's tolerance, not to the bit)."""
import ctypes as C

import numpy as np
import pytest

import wdbins_check as bc
import wdbins_ref as br
import wdmoments_check as wc
import wdmoments_ref as wr
from base_amd import abi, synth
from conftest import build_problem
from cli_util import cli as _cli, read_phot as _read_phot

pytestmark = pytest.mark.gpu
_dp = C.POINTER(C.c_double)
ALL = abi.WQ_ALL


class engine_for:
    """with engine_for(pack_d, cl, priors, ...) as eng: a short-lived engine on the dicts of a problem."""

    def __init__(self, pack_d, cl, priors, n_pops=1, K=1, n_q=1, mode=abi.MODE_GIVEN_MASS):
        self.args = (abi.make_pack(pack_d), abi.make_stars(cl), priors,
                     abi.make_options(mode=mode, n_pops=n_pops, marg_iso_increm=K, marg_n_q=n_q))

    def __enter__(self):
        from base_amd import engine
        self.eng = engine.Engine(*self.args)
        return self.eng

    def __exit__(self, *exc):
        self.eng.close()


def outside(pack_d, row):
    out = np.array(row, dtype=np.float64)
    out[abi.P_LOGAGE] = pack_d["log_age"][-1] + 1.0
    return out


def small_case(n_filt=8, n_pops=1, keep=13, name="parsec", n_rows=6, n_nodes=64):
    """(pack_d, cl, priors, rows, lines_by_row, edges [keep, 6, 31]) of a small WD-stage catalogue."""
    pack_d, cl, priors = wc.wd_problem(name, n_filt, 400, n_y=3 if n_pops == 2 else 1, n_pops=n_pops, keep=keep)
    rows = wc.rows_for(cl, n_rows, 3, n_pops)
    lines = [br.row_lines(pack_d, cl, par, n_pops, n_nodes) for par in rows]
    edges, _, margin = bc.own_edges(lines, rows, keep, ALL)
    assert np.all(margin >= bc.MARGIN)
    return pack_d, cl, priors, rows, lines, edges


# ---- 1. parity with the reference --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["parsec", "dsed", "girardi"])
def test_parity_with_the_reference(key):
    pack_d, cl, priors, rows, n_pops, n_nodes, x16 = wc.parity_fixture(key)[:7]
    lines, edges, _, margin = bc.parity_lines(key)
    assert np.all(margin >= bc.MARGIN)
    with engine_for(pack_d, cl, priors, n_pops) as eng:
        for n_bins in (1, 2, 30):
            e = bc.sub_edges(edges, n_bins)
            x = bc.reference_rows(lines, 150, ALL, e)
            for r in range(len(rows)):                                   # per row: one call per row, from zeros
                acc, idx = eng.wd_bins(rows[r], n_nodes, e)
                assert acc.shape == (150, 6, n_bins + 3)
                bc.assert_close(acc, x[r], f"{key}, {n_bins} bins, row {r}")
            assert np.array_equal(idx, np.arange(150))
            total, _ = eng.wd_bins(np.concatenate([rows, outside(pack_d, rows[0])[None]]), n_nodes, e)      # summed
            bc.assert_close(total, bc.summed(x), f"{key}, {n_bins} bins, summed")
            inner, C = bc.inner_bins_with_mass(total)
            assert n_bins < 30 or (inner[C > 0] >= 3).mean() >= 0.9
        none, _ = eng.wd_bins(outside(pack_d, rows[0]), n_nodes, edges)      # a row outside the grid adds nothing
        assert np.all(none == 0)
        both, _ = eng.wd_bins(np.stack([rows[2], outside(pack_d, rows[0])]), n_nodes, edges)
        assert np.array_equal(both, eng.wd_bins(rows[2], n_nodes, edges)[0])


# ---- 2. every instance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pops", [1, 2])
@pytest.mark.parametrize("n_filt", [3, 8, 16])
def test_every_instance(n_filt, n_pops):
    pack_d, cl, priors, rows, lines, edges = small_case(n_filt, n_pops, keep=22, name="dsed", n_rows=2)
    if n_pops == 2:
        assert np.all((rows[:, abi.P_LAMBDA] > 0) & (rows[:, abi.P_LAMBDA] < 1))
    with engine_for(pack_d, cl, priors, n_pops) as eng:
        acc, idx = eng.wd_bins(rows, 64, edges)
    want = bc.summed(bc.reference_rows(lines, 22, ALL, edges))
    assert len(idx) == 22 and (want[..., -1] > 0).sum() >= 6 * 15
    bc.assert_close(acc, want, f"{n_filt} filters, {n_pops} populations")


# ---- 3. the seams on the device's own bits -----------------------------------------------------------------------------------
def test_seams_on_device_bits():
    """v*: a drawn node's value as b9_sample_wd_mass reports it (zams, wd_mass, log_cool_age).  With an edge AT v* the node lies
    in the column above the edge (bins are closed on the left); with the edge one ulp higher its weight -- the reference's p w
    of that node -- has moved down one column; one ulp lower nothing changes, bit for bit.  For an inner edge, for e_0 and for
    e_B.  The other lines do not move at all."""
    pack_d, cl, priors, rows, lines, _ = small_case(keep=13)
    row, n_nodes = rows[:1], 64
    with engine_for(pack_d, cl, priors) as eng:
        g = eng.sample_wd_mass(row, n_nodes, seed=5)
        pick = None
        for i in np.flatnonzero((g["member"][0] > 0.5) & (g["log_teff"][0] != 0)):
            if lines[0][i] is None:
                continue
            p, w, m, cooled, der = lines[0][i]
            at = np.abs(m - g["zams"][0, i]) <= 1e-12 * m
            if at.sum() == 1 and cooled[at][0] and p * w[at][0] > 1e-3:
                pick, moved_ref = int(i), float(p * w[at][0])
                break
        assert pick is not None
        base = np.tile(np.array([-1000.0, 0.0, 1000.0]), (13, 6, 1))
        for q, key in ((abi.WQ_ZAMS, "zams"), (abi.WQ_WDMASS, "wd_mass"), (abi.WQ_LOGCOOL, "log_cool_age")):
            v = float(g[key][0, pick])
            up, down = np.nextafter(v, np.inf), np.nextafter(v, -np.inf)
            d = 0.5 * abs(v) + 1.0

            def h(e):
                edges = base.copy()
                edges[pick, q] = e
                return eng.wd_bins(row, n_nodes, edges)[0]

            for name, e_of, c_hi in (("inner", lambda x: [v - d, x, v + d], 2), ("e_0", lambda x: [x, v + d, v + 2 * d], 1),
                                     ("e_B", lambda x: [v - 2 * d, v - d, x], 3)):
                at_edge, above, below = h(e_of(v)), h(e_of(up)), h(e_of(down))
                assert np.array_equal(below, at_edge), (key, name)
                moved = above[pick, q, c_hi - 1] - at_edge[pick, q, c_hi - 1]
                tol = 4 * np.finfo(float).eps * at_edge[pick, q, :4].sum()            # the subtraction's own rounding
                print(f"{key} {name}: star {pick}, v* = {v!r}, moved {moved!r}, reference {moved_ref!r}")
                assert moved == pytest.approx(moved_ref, rel=1e-9, abs=tol)
                assert at_edge[pick, q, c_hi] - above[pick, q, c_hi] == pytest.approx(moved_ref, rel=1e-9, abs=tol)
                others = np.ones((13, 6), dtype=bool)
                others[pick, q] = False
                assert np.array_equal(above[others], at_edge[others]) and above[pick, q, 4] == at_edge[pick, q, 4]


# ---- 4. ties ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pops", [1, 2])
def test_ties_to_wd_moments(n_pops):
    pack_d, cl, priors, rows, lines, edges = small_case(8 if n_pops == 1 else 5, n_pops, keep=40, name="parsec" if n_pops == 1 else "dsed")
    with engine_for(pack_d, cl, priors, n_pops) as eng:
        mom, _ = eng.wd_moments(rows, 64)
        acc, _ = eng.wd_bins(rows, 64, edges)
        wide = np.tile(np.array([-1e6, 1e6]), (40, 6, 1))
        one, _ = eng.wd_bins(rows, 64, wide)
    assert (mom[:, wr.MEMBER] > 0).sum() >= 25
    for s in range(6):
        assert np.array_equal(acc[:, s, 32], mom[:, wr.MEMBER]) and np.array_equal(one[:, s, 3], mom[:, wr.MEMBER])     # the total, bit for bit
    np.testing.assert_allclose(one[:, 0, 1], mom[:, wr.MEMBER], rtol=1e-12, atol=0)
    for s in range(1, 6):                                                 # one enclosing bin of a derived quantity: COOLED, bit for bit
        assert np.array_equal(one[:, s, 1], mom[:, wr.COOLED]), br.NAMES[s]
        assert np.all(one[:, s, 0] == 0) and np.all(one[:, s, 2] == 0)
    np.testing.assert_allclose(acc[:, 0, :32].sum(axis=1), mom[:, wr.MEMBER], rtol=1e-12, atol=0)
    for s in range(1, 6):
        np.testing.assert_allclose(acc[:, s, :32].sum(axis=1), mom[:, wr.COOLED], rtol=1e-12, atol=0)


def test_counted_mass_strictly_between_zero_and_the_total():
    pack_d, cl, priors, rows, n_nodes = wc.seam_fixture()
    lines = [br.row_lines(pack_d, cl, par, 1, n_nodes) for par in rows]
    edges, _, margin = bc.own_edges(lines, rows, 6, ALL)
    assert np.all(margin >= bc.MARGIN)
    with engine_for(pack_d, cl, priors) as eng:
        acc, _ = eng.wd_bins(rows, n_nodes, edges)
    bc.assert_close(acc, bc.summed(bc.reference_rows(lines, 6, ALL, edges)), "the seam fixture")
    share = acc[:, 1:, :32].sum(axis=2) / acc[:, 1:, 32]
    print("counted share of the total, derived quantities:", share[:, 0])
    assert np.all((share > 0) & (share < 1)) and np.sum((share[:, 0] > 0.01) & (share[:, 0] < 0.99)) >= 3
    np.testing.assert_allclose(acc[:, 0, :32].sum(axis=1), acc[:, 0, 32], rtol=1e-12)


@pytest.mark.parametrize("K", [1, 3])
def test_zams_columns_tie_to_star_bins(K):
    """At n_nodes = 8 K the grid is b9_star_bins' for a WD-stage star.  Another order of summation: not the same bits."""
    pack_d, cl, _, _, priors, _ = build_problem("dsed", 5, n_stars=300, wd_frac=0.1, n_y=3, n_pops=2, seed=12)
    rows = wc.rows_for(cl, 5, 3, 2)
    wd = wr.wd_stars(cl)
    lines = [br.row_lines(pack_d, cl, par, 2, 8 * K) for par in rows]
    e = bc.own_edges(lines, rows, len(wd), 1 << abi.WQ_ZAMS)[0]
    all_edges = np.tile(np.linspace(0.1, 8.0, 31), (300, 1))
    all_edges[wd] = e[:, 0]
    with engine_for(pack_d, cl, priors, 2, K, 2) as eng:
        eng.set_tuning(marg_no_pruning=1)
        theirs = eng.star_bins(rows, all_edges, abi.HQ_PRIMARY)[wd]
        mine, idx = eng.wd_bins(rows, 8 * K, e, 1 << abi.WQ_ZAMS)
    assert np.array_equal(idx, wd) and len(wd) == 30 and (mine[:, 0, 32] > 0).sum() >= 20
    print("largest relative difference:", np.max(np.abs(mine[:, 0] - theirs) / np.maximum(np.abs(theirs), 1e-300)))
    np.testing.assert_allclose(mine[:, 0], theirs, rtol=1e-12, atol=0)


# ---- 5. invariances, bit for bit -----------------------------------------------------------------------------------------------
def test_bitwise_invariances():
    """13 WD-stage stars x 64 nodes x 260 rows (the 6 rows tiled: one call crosses the 256-row chunk)."""
    from base_amd import engine
    pack_d, cl_full, _, _, priors, _ = build_problem("parsec", 8, n_stars=400, wd_frac=0.25, seed=12)
    wd = wr.wd_stars(cl_full)[:13]
    cl = wc.subset(cl_full, wd)
    rows6 = wc.rows_for(cl, 6, 3, 1)
    lines = [br.row_lines(pack_d, cl, par, 1, 64) for par in rows6]
    edges = bc.own_edges(lines, rows6, 13, ALL)[0]
    rows = np.ascontiguousarray(np.tile(rows6, (44, 1))[:260])
    with engine_for(pack_d, cl, priors, 1, 2, 2) as eng:
        whole, _ = eng.wd_bins(rows, 64, edges)
        assert (whole[..., 32] > 0).sum() >= 6 * 8
        bc.assert_close(whole[:, :, :], sum_tiled(bc.reference_rows(lines, 13, ALL, edges), 260), "260 rows")
        acc, _ = eng.wd_bins(rows[:1], 64, edges)
        acc, _ = eng.wd_bins(rows[1:257], 64, edges, acc=acc)
        acc, _ = eng.wd_bins(rows[257:], 64, edges, acc=acc)
        assert np.array_equal(acc, whole)                                   # 1 + 256 + 3 continued
        assert np.array_equal(eng.wd_bins(rows, 64, edges)[0], whole)       # a repeated call
        eng.wd_moments(rows[:5], 77)
        eng.star_bins(rows[:3], np.tile(np.linspace(0.1, 8.0, 5), (13, 1)))
        eng.pointwise(rows[:7])
        eng.wd_bins(rows[:3], 100, edges[:, :2, :3], (1 << 1) | (1 << 4))
        assert np.array_equal(eng.wd_bins(rows, 64, edges)[0], whole)       # after other calls on the context
        for i, s in ((0, 0), (5, 3), (12, 5)):                              # a line with every other line's edges replaced
            other = np.roll(edges.reshape(78, 31), 1, axis=0).reshape(13, 6, 31).copy()
            other[i, s] = edges[i, s]
            assert np.array_equal(eng.wd_bins(rows, 64, other)[0][i, s], whole[i, s]), (i, s)
        for q in range(6):                                                  # a quantity alone against itself inside the full mask
            alone, _ = eng.wd_bins(rows, 64, edges[:, q:q + 1], 1 << q)
            assert np.array_equal(alone[:, 0], whole[:, q]), br.NAMES[q]
        pair, _ = eng.wd_bins(rows, 64, edges[:, [1, 4]], (1 << 1) | (1 << 4))
        assert np.array_equal(pair, whole[:, [1, 4]])
    with engine_for(pack_d, cl, priors, 1, 2, 2) as eng:                    # a fresh context
        assert np.array_equal(eng.wd_bins(rows, 64, edges)[0], whole)
    for i in (0, 7):                                                        # a star alone in a catalogue
        with engine_for(pack_d, wc.subset(cl, np.array([i])), priors) as eng:
            assert np.array_equal(eng.wd_bins(rows, 64, edges[i:i + 1])[0][0], whole[i]), i
    ms = np.flatnonzero(np.asarray(cl_full["stage"]) != abi.STAGE_WD)[:50]  # ... and among main-sequence stars
    sel = np.sort(np.concatenate([wd, ms]))
    with engine_for(pack_d, wc.subset(cl_full, sel), priors) as eng:
        mixed, idx = eng.wd_bins(rows, 64, edges)
    assert np.array_equal(sel[idx], wd) and np.array_equal(mixed, whole)


def sum_tiled(x6, n_rows):
    want = np.zeros(x6.shape[1:])
    for r in range(n_rows):
        want = want + x6[r % len(x6)]
    return want


# ---- 6. lines that add nothing ----------------------------------------------------------------------------------------------------
def test_lines_that_add_nothing():
    pack_d, cl, priors, rows, lines, edges = small_case(keep=13)
    cl = dict(cl, obs=np.array(cl["obs"], dtype=np.float64))
    cl["obs"][4] = 1e200                                                    # every chi^2 overflows: no finite term
    with engine_for(pack_d, cl, priors) as eng:
        acc, _ = eng.wd_bins(rows, 64, edges)
        mixed, _ = eng.wd_bins(np.stack([outside(pack_d, rows[0]), rows[0], rows[1], outside(pack_d, rows[0])]), 64, edges)
        plain, _ = eng.wd_bins(rows[:2], 64, edges)
        only, _ = eng.wd_bins(outside(pack_d, rows[0]), 64, edges, acc=np.full((13, 6, 33), 7.25))
    assert np.all(acc[4] == 0) and (np.delete(acc, 4, axis=0)[..., 32] > 0).sum() >= 6 * 8
    assert np.array_equal(mixed, plain) and np.all(only == 7.25)
    lines4 = [[None if c == 4 else ln for c, ln in enumerate(row)] for row in lines]
    bc.assert_close(acc, bc.summed(bc.reference_rows(lines4, 13, ALL, edges)), "a star without a finite term")
    # a row whose AGB tips are not below M_wd_up adds nothing
    low = dict(pack_d, m_wd_up=0.5)
    with engine_for(low, cl, priors) as eng:
        assert eng.derive_isochrone(rows[0])[3] > 0.5
        assert np.all(eng.wd_bins(rows, 64, edges)[0] == 0)
    # no WD-stage star: B9_OK, nothing touched
    pack_n, cl_n, _, _, priors_n, _ = build_problem("parsec", 4, n_stars=50, wd_frac=0.0, seed=4)
    with engine_for(pack_n, cl_n, priors_n) as eng:
        assert eng.n_wd_stars() == 0
        r = np.ascontiguousarray(wc.rows_for(cl_n, 2, 1, 1))
        e, a = np.array([0.0, 1.0]), np.full(4, 7.25)
        assert eng.lib.b9_wd_bins(eng._ctx, r.ctypes.data_as(_dp), 2, 64, 1, e.ctypes.data_as(_dp), 1, 0, a.ctypes.data_as(_dp)) == abi.B9_OK
        assert np.all(a == 7.25)
        acc, idx = eng.wd_bins(r, 64, np.zeros((0, 6, 31)))
        assert acc.shape == (0, 6, 33) and idx.size == 0


# ---- 7. errors, and sampler blocks left alone ---------------------------------------------------------------------------------------
def test_errors_leave_acc_untouched():
    from base_amd import mcmc
    pack_d, cl, pack, stars, priors, options = build_problem("parsec", 8, n_stars=400, wd_frac=0.1, seed=4)
    from base_amd import engine
    eng = engine.Engine(pack, stars, priors, options)
    try:
        n_wd = eng.n_wd_stars()
        assert n_wd >= 20
        rows = np.ascontiguousarray(wc.rows_for(cl, 4, 1, 1))
        good = np.tile(np.linspace(-5.0, 12.0, 32), (n_wd, 6, 1))

        def call(n_rows=4, n_nodes=64, mask=ALL, edges=None, n_bins=24, acc=True, params=True, with_edges=True, ctx=True):
            n_sel = max(1, bin(mask & 63).count("1")) if 0 < mask < 64 else 6
            edges = np.ascontiguousarray(good[:, :n_sel, :25] if edges is None else edges, dtype=np.float64)
            a = np.full((n_wd, 6, 34), 7.25)
            rc = eng.lib.b9_wd_bins(eng._ctx if ctx else None, rows.ctypes.data_as(_dp) if params else None, n_rows, n_nodes, mask,
                                    edges.ctypes.data_as(_dp) if with_edges else None, n_bins, 0, a.ctypes.data_as(_dp) if acc else None)
            assert rc == abi.B9_OK or np.all(a == 7.25)
            assert rc != abi.B9_OK or not np.all(a == 7.25)
            return rc

        assert call() == abi.B9_OK and call(edges=good[:, :, :31], n_bins=30) == abi.B9_OK and call(edges=good[:, :, :2], n_bins=1) == abi.B9_OK
        assert call(mask=1 << 3) == abi.B9_OK and call(mask=5) == abi.B9_OK
        assert call(n_bins=0) == abi.B9_ERR_INVALID and call(n_bins=-1) == abi.B9_ERR_INVALID
        assert call(edges=good, n_bins=31) == abi.B9_ERR_INVALID
        assert call(mask=0) == abi.B9_ERR_INVALID and call(mask=64) == abi.B9_ERR_INVALID and call(mask=ALL | 128) == abi.B9_ERR_INVALID
        assert call(mask=-1) == abi.B9_ERR_INVALID
        assert call(n_nodes=0) == abi.B9_ERR_INVALID and call(n_nodes=-3) == abi.B9_ERR_INVALID
        assert call(n_rows=0) == abi.B9_ERR_INVALID and call(n_rows=-2) == abi.B9_ERR_INVALID
        assert call(acc=False) == abi.B9_ERR_INVALID and call(params=False) == abi.B9_ERR_INVALID and call(with_edges=False) == abi.B9_ERR_INVALID
        assert call(ctx=False) == abi.B9_ERR_INVALID
        assert call(edges=good[:, :, :25][:, :, ::-1]) == abi.B9_ERR_INVALID                      # descending
        for star, s, b, value in ((n_wd - 1, 5, 10, None), (0, 0, 24, np.nan), (7, 3, 0, np.inf), (11, 2, 3, -np.inf)):   # one bad edge in a single line
            e = good[:, :, :25].copy()
            e[star, s, b] = e[star, s, b - 1] if value is None else value                         # two equal; not finite
            assert call(edges=e) == abi.B9_ERR_INVALID
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


@pytest.mark.parametrize("mode", [abi.MODE_GIVEN_MASS, abi.MODE_MARGINALISED])
def test_sampler_blocks_are_untouched(mode):
    from base_amd import engine, mcmc
    pack_d, cl, pack, stars, priors, _ = build_problem("parsec", 8, n_stars=400, wd_frac=0.1, seed=4)
    options = abi.make_options(mode=mode, n_pops=1, marg_iso_increm=1, marg_n_q=4)
    free = np.array(mcmc.DEFAULT_FREE)
    chol = np.diag([mcmc.DEFAULT_STEP[k] for k in free]) * 0.3
    start = synth.walker_params(cl["truth"], 4, seed=2, scale=0.3)
    rows = wc.rows_for(cl, 3, 1, 1)
    n_wd = int((np.asarray(cl["stage"]) == abi.STAGE_WD).sum())
    edges = np.tile(np.linspace(-5.0, 12.0, 31), (n_wd, 6, 1))

    def run(interleave):
        eng = engine.Engine(pack, stars, priors, options)
        try:
            lp0 = eng.logpost(start)
            h = eng.mcmc_submit(start, lp0, np.arange(4), free, chol, 11, 0, 6, asynchronous=True)
            if interleave:
                with pytest.raises(engine.B9Error) as e:                   # B9_ERR_STATE: a block is outstanding
                    eng.wd_bins(rows, 64, edges)
                assert e.value.code == abi.B9_ERR_STATE and "outstanding" in str(e.value)
            first = [np.array(x) for x in eng.mcmc_collect(h)[:4]]
            if interleave:
                acc, _ = eng.wd_bins(rows, 64, edges)
                assert (acc[..., 32] > 0).sum() >= 6 * 10
            h = eng.mcmc_submit(start, lp0, np.arange(4), free, chol, 11, 6, 6, cont=True, asynchronous=True)
            second = [np.array(x) for x in eng.mcmc_collect(h)[:4]]
        finally:
            eng.close()
        return first + second

    for a, b in zip(run(False), run(True)):
        assert np.array_equal(a, b)


# ---- 8. end to end ----------------------------------------------------------------------------------------------------------------
def test_wd_intervals_end_to_end():
    """hostlib.wd_intervals with its defaults on the dsed fixture (150 WD-stage stars, two populations, 6 rows, 512 nodes): every
    bracket of every line with counted mass contains its level of the reference CDF within 1e-12, a bracket reported final is
    final, and at least 90 % of those lines are final at every level within 12 passes with lo(16 %) < hi(84 %); lines without
    counted mass carry NaN and the flag."""
    from base_amd import hostlib
    pack_d, cl, priors, rows, n_pops, n_nodes = wc.parity_fixture("dsed")[:6]
    lines = bc.parity_lines("dsed")[0]
    with engine_for(pack_d, cl, priors, n_pops) as eng:
        res = hostlib.wd_intervals(eng, rows, n_nodes)
        mom, _ = eng.wd_moments(rows, n_nodes)
    lv = res["levels"]
    assert tuple(lv) == hostlib.STAR_INTERVALS_LEVELS and res["n_passes"] <= 12 and res["n_wd"] == 150 and res["n_sel"] == 6
    has = bc.assert_brackets(lines, rows, 150, ALL, lv, res["lo"], res["hi"], res["final"], 1e-4, "dsed, defaults")
    good = has & res["final"].all(axis=1) & (res["lo"][:, 1] < res["hi"][:, 3])
    print(f"{int(good.sum())} of {int(has.sum())} lines final with lo(16 %) < hi(84 %) after {res['n_passes']} passes; passes used: {np.bincount(res['passes'])}")
    assert has.sum() >= 6 * 100 and good.sum() >= 0.9 * has.sum()
    assert np.all((res["value"][has] >= res["lo"][has]) & (res["value"][has] <= res["hi"][has]))
    assert np.all(np.diff(res["value"][has], axis=1) >= 0)
    none = ~has
    assert np.all(res["flags"][none] == hostlib.SIV_NO_MASS) and np.isnan(res["value"][none]).all()
    assert np.array_equal(res["member"].reshape(150, 6)[:, 0], mom[:, wr.MEMBER] / 6)
    counted = res["counted"].reshape(150, 6)
    mem = mom[:, wr.MEMBER] > 0
    np.testing.assert_allclose(counted[mem, 0], 1.0, rtol=1e-12)
    np.testing.assert_allclose(counted[mem, 1:], np.repeat((mom[mem, wr.COOLED] / mom[mem, wr.MEMBER])[:, None], 5, axis=1), rtol=1e-12, atol=1e-300)


def test_cli_wd_intervals(tmp_path):
    """The wdIntervals program on a 40-star WD-stage catalogue and 6 rows, read from files: the file parses and equals, number for
    number, hostlib.wd_intervals_table(hostlib.wd_intervals(..)) on a context loaded from the same files; a second run with
    other flags likewise."""
    from base_amd import build, engine, host_build, hostlib
    build.build_hip()
    host_build.build_host()
    pack_d, cl, priors = wc.wd_problem("parsec", 8, 400, keep=40)
    rows = wc.rows_for(cl, 6, 3, 1)
    truth = np.array(cl["truth"])
    root = synth.write_models_dir(pack_d, str(tmp_path / "models"))
    base = str(tmp_path / "run")
    synth.write_phot(cl, pack_d["filters"], base + ".phot")
    y = synth.write_yaml(str(tmp_path / "run.yaml"), base + ".phot", root, base, truth, ms_model=pack_d.get("name", "parsec"))
    names = ["logAge", "Y", "FeH", "modulus", "absorption", "carbonicity", "IFMRconst", "IFMRlin", "IFMRquad"]
    with open(base + ".res", "w") as f:
        f.write(" ".join(names) + " logPost stage\n")
        for r in rows:
            f.write(" ".join(repr(float(x)) for x in r[:9]) + " -1.0 3\n")
    r = _cli("wdIntervals", "--config", y, "--nMassNodes", "64")
    assert r.returncode == 0, r.stderr
    assert "passes" in r.stderr and "lines unfinished" in r.stderr and "6 quantities" in r.stderr

    cl_f = _read_phot(base + ".phot")
    got_rows = hostlib.read_res_rows(base + ".res", truth, 3)
    assert np.array_equal(got_rows[:, :9], rows[:, :9]) and len(got_rows) == 6
    eng = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cl_f), priors, wc.opts())
    try:
        res = hostlib.wd_intervals(eng, got_rows, 64)
        res2 = hostlib.wd_intervals(eng, got_rows, 64, ("logCoolAge", "zamsMass"), (0.1, 0.9), 1e-3, 4)
    finally:
        eng.close()
    ids, cols, tab = hostlib.read_wd_intervals(base + ".wdIntervals")
    want = hostlib.wd_intervals_table(res)
    assert ids == [str(i + 1) for i in range(40)]
    want_cols = ["member"]
    for n in hostlib.WD_QUANTITY_NAMES:
        want_cols += [n + "_counted"] + [f"{n}_q{a:.12g}{s}" for a in hostlib.STAR_INTERVALS_LEVELS for s in ("", "_lo", "_hi")] + [n + "_passes", n + "_flags"]
    assert cols == want_cols
    assert tab.shape == want.shape == (40, 1 + 6 * 18) and np.array_equal(tab, want, equal_nan=True)
    has = ~np.isnan(want[:, 2])
    assert has.sum() >= 25 and np.all(want[has, 17] <= 12)

    r = _cli("wdIntervals", "--config", y, "--nMassNodes", "64", "--quantities", "logCoolAge,zamsMass", "--levels", "0.1,0.9", "--tol", "1e-3",
             "--maxPasses", "4")
    assert r.returncode == 0, r.stderr
    _, cols2, tab2 = hostlib.read_wd_intervals(base + ".wdIntervals")
    assert cols2 == ["member"] + [f"{n}_{c}" for n in ("zamsMass", "logCoolAge")
                                  for c in ("counted", "q0.1", "q0.1_lo", "q0.1_hi", "q0.9", "q0.9_lo", "q0.9_hi", "passes", "flags")]
    assert np.array_equal(tab2, hostlib.wd_intervals_table(res2), equal_nan=True)
    assert np.all(tab2[:, [8, 17]] <= 4)
