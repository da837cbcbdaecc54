"""b9_star_bins (the starIntervals counterpart) on the GPU: the accumulators on per-star edges against the numpy statement
tests/starbins_ref.py, the bin seams on the device's own bits, the bit-for-bit contract (b9_mass_hist's bins on shared edges,
b9_star_moments' membership, chunking, continuation, call history, the other stars' edges, the other stars), rows and stars
that add nothing, the errors, every kernel instance, and star_intervals end to end with the starIntervals program.

The catalogue is dsed, 5 filters, 130 stars -- three 64-star chunks, the last one partial -- of which 13 are WD-stage -- a
partial four-wave workgroup --, on a 2 x 2 grid, with one and with two populations at lambda = 0.3, over 3 rows and over 34
(one call crosses the 32-row chunk).  A case's reference nodes are computed once and shared.

Tolerance of every comparison with the reference: masshist_check.assert_star_hist's (rtol 1e-9, atol N_nodes e^-40 per row),
for every column.  A star's edges are its own weighted quantiles between the 5 % and the 95 % point, separated from every node
value of that star by 1e-9 relative (the device forms M1 by fma, numpy by two roundings)."""
import ctypes as C
import functools

import numpy as np
import pytest

import masshist_check as hc
import masshist_ref as hr
import moments_ref as mr
import starbins_check as sc
import starbins_ref as sr
import test_gpu_moments as tm
from base_amd import abi, synth
from conftest import build_problem
from cli_util import cli as _cli

pytestmark = pytest.mark.gpu

QUANTITIES = [abi.HQ_PRIMARY, abi.HQ_SECONDARY, abi.HQ_SYSTEM]
QNAMES = {abi.HQ_PRIMARY: "primary", abi.HQ_SECONDARY: "secondary", abi.HQ_SYSTEM: "system"}
K, Q, N_NODES = 2, 2, {1: 356, 2: 712}                 # N_nodes = pops * 89 EEP intervals * K * Q
_dp = C.POINTER(C.c_double)


def make_engine(pack, stars, priors, n_pops, mode=abi.MODE_GIVEN_MASS, k=K, q=Q):
    from base_amd import engine
    return engine.Engine(pack, stars, priors, tm.opts(n_pops, k, q, mode))


@functools.lru_cache(maxsize=None)
def case(n_pops):
    """The 130-star catalogue with its 34 rows (lambda = 0.3) and the reference's nodes of every row, built once."""
    pack_d, cl, pack, stars, priors, _ = build_problem("dsed", 5, n_stars=130, wd_frac=0.1, n_y=3, n_pops=n_pops, seed=12)
    rows = synth.walker_params(cl["truth"], 34, seed=3, scale=0.3, n_pops=n_pops)
    rows[:, abi.P_LAMBDA] = 0.3
    rows.setflags(write=False)
    wd = np.asarray(cl["stage"]) == abi.STAGE_WD
    assert 5 <= wd.sum() <= 15 and wd.sum() % 4 != 0
    return pack_d, cl, pack, stars, priors, rows, hr.nodes_of_rows(pack_d, cl, rows, n_pops, K, Q)


@functools.lru_cache(maxsize=None)
def case_edges(n_pops, n_rows, quantity, n_bins):
    """The case's per-star edges (from the reference's nodes of the rows used), with five stars given special ones: every node
    below e_0; every node at or above e_B (an MS/RGB and a WD-stage star); edges that are adjacent doubles (likewise)."""
    pack_d, cl, pack, stars, priors, rows, nodes = case(n_pops)
    edges = sc.own_edges(cl, nodes[:n_rows], quantity, n_bins)
    wd = np.asarray(cl["stage"]) == abi.STAGE_WD
    ms_i, wd_i = np.flatnonzero(~wd), np.flatnonzero(wd)
    v, _ = hc.reference_values(nodes[:n_rows], quantity)
    vmax, vmin = (v.max(), v.min()) if len(v) else (8.0, 0.1)
    edges[ms_i[1]] = np.linspace(1.5 * vmax, 2.0 * vmax, n_bins + 1)         # all below
    for i in (ms_i[70], wd_i[2]):
        edges[i] = np.linspace(0.25 * vmin, 0.5 * vmin, n_bins + 1)          # all at or above
    for i in (ms_i[66], wd_i[0]):                                            # adjacent doubles, from an edge no node is near
        e = edges[i, n_bins // 2]
        for b in range(n_bins + 1):
            edges[i, b] = e
            e = np.nextafter(e, np.inf)
    assert np.all(np.diff(edges, axis=1) > 0)
    edges.setflags(write=False)
    return edges


# ---- 1. parity with the reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins", [1, 2, 30])
@pytest.mark.parametrize("n_rows", [3, 34])
@pytest.mark.parametrize("n_pops", [1, 2])
def test_parity_with_reference(n_pops, n_rows, n_bins):
    """Every column of every star against the reference, the three quantities.  Non-vacuity, from the reference alone:
    masshist_check.non_vacuity's condition (at least half of the live stars have two or more columns above 1e-3 of their
    total) in every case; and with 30 bins over 34 rows at least 90 % of the stars with counted mass have mass in three or
    more of their OWN bins (figures of the reference, PRIMARY SECONDARY SYSTEM: one population 119 104 119 of 124 113 124;
    two populations 122 112 122 of 127 116 127 -- the five stars with special edges among those that do not).  Over 3 rows a
    star's posterior sits on too few nodes for that (45 of 124), and one or two bins cannot hold three: there the first
    condition alone is asserted."""
    pack_d, cl, pack, stars, priors, rows, nodes = case(n_pops)
    rows, nodes = rows[:n_rows], nodes[:n_rows]
    wd = np.asarray(cl["stage"]) == abi.STAGE_WD
    eng = make_engine(pack, stars, priors, n_pops)
    try:
        for quantity in QUANTITIES:
            edges = case_edges(n_pops, n_rows, quantity, n_bins)
            want = sr.accumulate(pack_d, cl, rows, n_pops, K, Q, quantity, edges, nodes_by_row=nodes)
            live, two, _ = hc.non_vacuity(want, n_rows)
            k, counted = sc.bins_with_mass(want)
            has = counted > 0
            print(f"{QNAMES[quantity]}: {live} live, {two} with two or more columns, {int((k[has] >= 3).sum())} of {int(has.sum())} with three or more own bins")
            assert live >= 120 and two >= (live + 1) // 2
            if n_bins == 30 and n_rows == 34:
                assert (k[has] >= 3).sum() >= 0.9 * has.sum()
            got = eng.star_bins(rows, edges, quantity)
            sc.assert_star_bins(got, want, N_NODES[n_pops], n_rows, f"{n_pops} pops, {n_rows} rows, {n_bins} bins, {QNAMES[quantity]}")
            if quantity == abi.HQ_SECONDARY:                 # the WD-stage stars: the total column only
                assert np.all(got[wd, :n_bins + 2] == 0) and np.any(got[wd, n_bins + 2] > 0)
            else:
                i_below, i_above = np.flatnonzero(~wd)[1], np.flatnonzero(~wd)[70]
                assert got[i_below, 0] > 0 and np.all(got[i_below, 1:n_bins + 2] == 0)
                assert got[i_above, n_bins + 1] > 0 and np.all(got[i_above, :n_bins + 1] == 0)
    finally:
        eng.close()


@pytest.mark.parametrize("n_pops", [1, 2])
@pytest.mark.parametrize("n_filt", [3, 8, 16])
def test_every_instance(n_filt, n_pops):
    pack_d, cl, pack, stars, priors, _ = build_problem("dsed", n_filt, n_stars=70, wd_frac=0.1, n_y=3, n_pops=n_pops, seed=12)
    rows = tm.rows_for(pack_d, cl, n_pops, 2, outside=False)
    rows[:, abi.P_LAMBDA] = 0.3
    nodes = hr.nodes_of_rows(pack_d, cl, rows, n_pops, K, Q)
    edges = sc.own_edges(cl, nodes, abi.HQ_SYSTEM, 30)
    eng = make_engine(pack, stars, priors, n_pops)
    try:
        got = eng.star_bins(rows, edges, abi.HQ_SYSTEM)
    finally:
        eng.close()
    want = sr.accumulate(pack_d, cl, rows, n_pops, K, Q, abi.HQ_SYSTEM, edges, nodes_by_row=nodes)
    assert (want[:, 32] > 0).sum() >= 60
    sc.assert_star_bins(got, want, tm.n_nodes_of(pack_d, n_pops, K, Q), 2, f"{n_filt} filters, {n_pops} pops")


# ---- 2. the seams on the device's own bits ----------------------------------------------------------------------------------
@pytest.mark.parametrize("stage", ["ms", "wd"])
def test_seams_on_device_bits(stage):
    """m*: a node mass as b9_sample_mass reports it.  With an edge AT m* the node lies in the column above the edge (bins are
    closed on the left); with the edge one ulp higher its weight -- the reference's p sum w over its nodes within 1e-12
    relative of m* -- has moved to the column below; one ulp lower nothing changes, bit for bit.  For an inner edge, for e_0
    (below <-> bin 0) and for e_B (the last bin <-> at or above).  The other stars' lines do not move at all."""
    pack_d, cl, pack, stars, priors, rows, nodes = case(1)
    row = rows[:1]
    is_wd = np.asarray(cl["stage"]) == abi.STAGE_WD
    want = is_wd if stage == "wd" else ~is_wd
    eng = make_engine(pack, stars, priors, 1)
    try:
        mass, ratio, member, pop = eng.sample_mass(row, seed=5)
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
        base = np.tile(np.array([0.05, 0.5, 20.0]), (eng.n_stars, 1))

        def h(e):
            edges = base.copy()
            edges[pick] = e
            return eng.star_bins(row, edges, abi.HQ_PRIMARY)

        for name, e_of, c_hi in (("inner", lambda x: [0.5 * m, x, 2.0 * m], 2), ("e_0", lambda x: [x, 1.5 * m, 2.0 * m], 1), ("e_B", lambda x: [0.25 * m, 0.5 * m, x], 3)):
            at_edge, above, below = h(e_of(m)), h(e_of(up)), h(e_of(down))
            assert np.array_equal(below, at_edge), name
            moved = above[pick, c_hi - 1] - at_edge[pick, c_hi - 1]
            tol = 4 * np.finfo(float).eps * at_edge[pick, :4].sum()               # the subtraction's own rounding
            print(f"{stage} {name}: star {pick}, m* = {m!r}, moved {moved!r}, reference {moved_ref!r}")
            assert moved == pytest.approx(moved_ref, rel=1e-9, abs=tol)
            assert at_edge[pick, c_hi] - above[pick, c_hi] == pytest.approx(moved_ref, rel=1e-9, abs=tol)
            others = np.arange(eng.n_stars) != pick
            assert np.array_equal(above[others], at_edge[others]) and np.array_equal(above[pick, 4], at_edge[pick, 4])
    finally:
        eng.close()


# ---- 3. the bitwise contract ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pops", [1, 2])
def test_shared_edges_are_mass_hist_bits(n_pops):
    """Identical edges for every star: columns 1 .. B and the total are b9_mass_hist's star_hist, bit for bit; the total is
    b9_star_moments' B9_MOM_MEMBER, bit for bit; and the columns of a star sum to its total where every node counts."""
    pack_d, cl, pack, stars, priors, rows, nodes = case(n_pops)
    eng = make_engine(pack, stars, priors, n_pops)
    try:
        member = eng.star_moments(rows)[:, abi.MOM_MEMBER]
        assert (member > 1.0).sum() >= 100
        for quantity in QUANTITIES:
            for n_bins in (1, 2, 30):
                # the first and the last of n_bins + 2 bins of equal posterior weight are cut off: by construction some star has
                # weight below e_0 and some star at or above e_B, so the two open columns are not columns of zeros
                shared = hc.quantile_edges(nodes, quantity, n_bins + 2)[1:-1]
                acc = eng.star_bins(rows, np.tile(shared, (eng.n_stars, 1)), quantity)
                star_hist, _ = eng.mass_hist(rows, shared, quantity, want_rows=False)
                assert np.array_equal(acc[:, 1:n_bins + 1], star_hist[:, :n_bins]), (QNAMES[quantity], n_bins)
                assert np.array_equal(acc[:, n_bins + 2], star_hist[:, n_bins])
                assert np.array_equal(acc[:, n_bins + 2], member)
                assert (acc[:, 0] > 0).any() and (acc[:, n_bins + 1] > 0).any()
                if quantity != abi.HQ_SECONDARY:
                    np.testing.assert_allclose(acc[:, :n_bins + 2].sum(axis=1), member, rtol=1e-12, atol=34 * N_NODES[n_pops] * np.exp(-40.0))
    finally:
        eng.close()


def test_bitwise_invariances():
    """34 rows in one call = 1 + 32 + 1 continued; a repeated call; a call after b9_mass_hist / b9_pointwise on the same
    context; a fresh context; star i's line with every other star's edges replaced; star i alone in a catalogue."""
    from base_amd import engine
    pack_d, cl, pack, stars, priors, rows, nodes = case(2)
    q, B = abi.HQ_SYSTEM, 30
    edges = case_edges(2, 34, q, B)
    is_wd = np.asarray(cl["stage"]) == abi.STAGE_WD
    eng = make_engine(pack, stars, priors, 2)
    try:
        whole = eng.star_bins(rows, edges, q)
        assert (whole[:, B + 2] > 0).sum() >= 120
        acc = eng.star_bins(rows[:1], edges, q)
        acc = eng.star_bins(rows[1:33], edges, q, acc)
        acc = eng.star_bins(rows[33:], edges, q, acc)
        assert np.array_equal(acc, whole)
        assert np.array_equal(eng.star_bins(rows, edges, q), whole)
        eng.mass_hist(rows[:5], np.linspace(0.1, 8.0, 41), abi.HQ_PRIMARY)
        eng.pointwise(rows[:7])
        eng.star_bins(rows[:3], edges[:, :3], abi.HQ_SECONDARY)
        assert np.array_equal(eng.star_bins(rows, edges, q), whole)
        # the other stars' edges: every star but i gets other valid ones (its neighbour's)
        for i in (int(np.flatnonzero(~is_wd)[5]), int(np.flatnonzero(~is_wd)[100]), int(np.flatnonzero(is_wd)[3])):
            other = np.roll(edges, 1, axis=0)
            other[i] = edges[i]
            assert np.array_equal(eng.star_bins(rows, other, q)[i], whole[i]), i
    finally:
        eng.close()
    eng = make_engine(pack, stars, priors, 2)                               # a fresh context
    try:
        assert np.array_equal(eng.star_bins(rows, edges, q), whole)
    finally:
        eng.close()
    for i in (int(np.flatnonzero(~is_wd)[5]), int(np.flatnonzero(~is_wd)[100]), int(np.flatnonzero(is_wd)[3])):
        eng = engine.Engine(pack, abi.make_stars(tm.subset(cl, np.array([i]))), priors, tm.opts(2, K, Q))
        try:
            assert np.array_equal(eng.star_bins(rows, edges[i:i + 1], q)[0], whole[i]), i
        finally:
            eng.close()


@pytest.mark.parametrize("mode", [abi.MODE_GIVEN_MASS, abi.MODE_MARGINALISED])
def test_sampler_blocks_are_untouched(mode):
    from base_amd import mcmc
    pack_d, cl, pack, stars, priors, rows, nodes = case(1)
    free = np.array(mcmc.DEFAULT_FREE)
    chol = np.diag([mcmc.DEFAULT_STEP[k] for k in free]) * 0.3
    start = synth.walker_params(cl["truth"], 4, seed=2, scale=0.3)
    edges = case_edges(1, 3, abi.HQ_PRIMARY, 30)

    def run(interleave):
        eng = make_engine(pack, stars, priors, 1, mode, 1, 4)
        try:
            lp0 = eng.logpost(start)
            h = eng.mcmc_submit(start, lp0, np.arange(4), free, chol, 11, 0, 6, asynchronous=True)
            if interleave:
                with pytest.raises(Exception) as e:                        # B9_ERR_STATE: a block is outstanding
                    eng.star_bins(rows[:3], edges)
                assert e.value.code == abi.B9_ERR_STATE and "outstanding" in str(e.value)
            first = [np.array(x) for x in eng.mcmc_collect(h)[:4]]
            if interleave:
                acc = eng.star_bins(rows[:3], edges)
                assert (acc[:, 32] > 0).sum() >= 100
            h = eng.mcmc_submit(start, lp0, np.arange(4), free, chol, 11, 6, 6, cont=True, asynchronous=True)
            second = [np.array(x) for x in eng.mcmc_collect(h)[:4]]
        finally:
            eng.close()
        return first + second

    for a, b in zip(run(False), run(True)):
        assert np.array_equal(a, b)


# ---- 4. rows and stars that add nothing -------------------------------------------------------------------------------------
def test_rows_and_stars_that_add_nothing():
    """A row outside the grid adds nothing, wherever it stands; a star with no live node (an observation no node is near in
    fp64: every chi^2 overflows) has every entry 0 -- the total too."""
    pack_d, cl, pack, _, priors, rows, nodes = case(2)
    cl = tm.subset(cl, np.arange(130))
    cl["obs"] = np.array(cl["obs"], dtype=np.float64)
    is_wd = np.asarray(cl["stage"]) == abi.STAGE_WD
    gone = [int(np.flatnonzero(~is_wd)[9]), int(np.flatnonzero(is_wd)[4])]
    for i in gone:
        cl["obs"][i] = 1e200
    outside = np.array(rows[0]); outside[abi.P_LOGAGE] = pack_d["log_age"][-1] + 1.0
    edges = np.array(case_edges(2, 3, abi.HQ_PRIMARY, 30))
    eng = make_engine(pack, abi.make_stars(cl), priors, 2)
    try:
        plain = eng.star_bins(rows[:3], edges, abi.HQ_PRIMARY)
        mixed = eng.star_bins(np.stack([outside, rows[0], rows[1], outside, rows[2], outside]), edges, abi.HQ_PRIMARY)
        only = eng.star_bins(np.stack([outside, outside]), edges, abi.HQ_PRIMARY, np.full_like(plain, 7.25))
    finally:
        eng.close()
    assert np.array_equal(mixed, plain) and np.all(only == 7.25)
    want = sr.accumulate(pack_d, cl, rows[:3], 2, K, Q, abi.HQ_PRIMARY, edges)
    assert np.all(want[gone] == 0) and (want[:, 32] > 0).sum() >= 120
    assert np.all(plain[gone] == 0) and np.array_equal(plain[:, 32] > 0, want[:, 32] > 0)
    sc.assert_star_bins(plain, want, N_NODES[2], 3, "two stars without a live node")


# ---- 5. errors ----------------------------------------------------------------------------------------------------------------
def test_errors_leave_acc_untouched():
    from base_amd import mcmc
    pack_d, cl, pack, stars, priors, rows, nodes = case(1)
    eng = make_engine(pack, stars, priors, 1)
    try:
        n = eng.n_stars
        rows = np.ascontiguousarray(rows[:4])
        good = np.tile(np.linspace(0.1, 8.0, 32), (n, 1))

        def call(n_rows=4, quantity=abi.HQ_PRIMARY, edges=good[:, :25], n_bins=24, acc=True, params=True, with_edges=True):
            edges = np.ascontiguousarray(edges, dtype=np.float64)
            a = np.full((n, 34), 7.25)
            rc = eng.lib.b9_star_bins(eng._ctx, rows.ctypes.data_as(_dp) if params else None, n_rows, quantity,
                                      edges.ctypes.data_as(_dp) if with_edges else None, n_bins, 0, a.ctypes.data_as(_dp) if acc else None)
            assert rc == abi.B9_OK or np.all(a == 7.25)
            assert rc != abi.B9_OK or not np.all(a == 7.25)
            return rc

        assert call() == abi.B9_OK and call(edges=good[:, :31], n_bins=30) == abi.B9_OK and call(edges=good[:, :2], n_bins=1) == abi.B9_OK
        assert call(n_bins=0) == abi.B9_ERR_INVALID and call(n_bins=-1) == abi.B9_ERR_INVALID
        assert call(edges=good, n_bins=31) == abi.B9_ERR_INVALID
        assert call(edges=good[:, :25][:, ::-1]) == abi.B9_ERR_INVALID                        # descending
        for star, b, value in ((57, 10, None), (0, 24, np.nan), (129, 0, np.inf), (64, 3, -np.inf)):   # a single star's edges
            e = good[:, :25].copy()
            e[star, b] = e[star, b - 1] if value is None else value                              # two equal; not finite
            assert call(edges=e) == abi.B9_ERR_INVALID
        assert call(quantity=3) == abi.B9_ERR_INVALID and call(quantity=-1) == abi.B9_ERR_INVALID
        assert call(n_rows=0) == abi.B9_ERR_INVALID and call(n_rows=-2) == abi.B9_ERR_INVALID
        assert call(acc=False) == abi.B9_ERR_INVALID and call(params=False) == abi.B9_ERR_INVALID and call(with_edges=False) == abi.B9_ERR_INVALID
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


# ---- 6. end to end --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quantity", QUANTITIES, ids=[QNAMES[q] for q in QUANTITIES])
@pytest.mark.parametrize("n_pops", [1, 2])
def test_star_intervals_end_to_end(n_pops, quantity):
    """hostlib.star_intervals over the 34 rows with its defaults: every bracket of every star with counted mass contains its
    level of the reference CDF of the full (row x node) mixture within 1e-12, a bracket reported final is final, and at least
    90 % of those stars are final at every level within the default passes with lo(16 %) < hi(84 %).  The stars without
    counted mass (WD-stage under SECONDARY, stars with no weight) carry NaN and the flag."""
    from base_amd import hostlib
    pack_d, cl, pack, stars, priors, rows, nodes = case(n_pops)
    eng = make_engine(pack, stars, priors, n_pops)
    try:
        assert eng.max_mass == max(float(np.max(pack_d["mass"])), float(pack_d["m_wd_up"]))
        res = hostlib.star_intervals(eng, rows, quantity)
    finally:
        eng.close()
    lv = res["levels"]
    assert tuple(lv) == hostlib.STAR_INTERVALS_LEVELS and res["n_passes"] <= 12
    has = sc.assert_brackets(cl, nodes, quantity, lv, res["lo"], res["hi"], res["final"], 1e-4, f"{n_pops} pops, {QNAMES[quantity]}")
    good = has & res["final"].all(axis=1) & (res["lo"][:, 1] < res["hi"][:, 3])
    print(f"{int(good.sum())} of {int(has.sum())} stars final with lo(16 %) < hi(84 %) after {res['n_passes']} passes; passes used: {np.bincount(res['passes'])}")
    assert has.sum() >= 110 and good.sum() >= 0.9 * has.sum()
    assert np.all((res["value"][has] >= res["lo"][has]) & (res["value"][has] <= res["hi"][has]))
    assert np.all(np.diff(res["value"][has], axis=1) >= 0)
    none = ~has
    assert np.all(res["flags"][none] == hostlib.SIV_NO_MASS) and np.isnan(res["value"][none]).all()
    if quantity == abi.HQ_SECONDARY:
        assert none[np.asarray(cl["stage"]) == abi.STAGE_WD].all()
    np.testing.assert_allclose(res["member"], mr.accumulate(pack_d, cl, rows, n_pops, K, Q)[:, abi.MOM_MEMBER] / 34, rtol=1e-9, atol=N_NODES[n_pops] * np.exp(-40.0))


def test_cli_star_intervals(tmp_path):
    """The starIntervals program on the 130-star catalogue and its 34 rows (one population), read from files: the file parses and
    equals, number for number, hostlib.star_intervals_table(hostlib.star_intervals(..)) on a context loaded from the same
    files; a second run with other flags likewise."""
    from base_amd import build, engine, host_build, hostlib
    build.build_hip()
    host_build.build_host()
    pack_d, cl, pack, stars, priors, rows, nodes = case(1)
    truth = np.array(cl["truth"])
    root = synth.write_models_dir(pack_d, str(tmp_path / "models"))
    base = str(tmp_path / "run")
    synth.write_phot(cl, pack_d["filters"], base + ".phot")
    y = synth.write_yaml(str(tmp_path / "run.yaml"), base + ".phot", root, base, truth, ms_model=pack_d.get("name", "dsed"))
    names = ["logAge", "Y", "FeH", "modulus", "absorption", "carbonicity", "IFMRconst", "IFMRlin", "IFMRquad"]
    with open(base + ".res", "w") as f:
        f.write(" ".join(names) + " logPost stage\n")
        for r in rows:
            f.write(" ".join(repr(float(x)) for x in r[:9]) + " -1.0 3\n")
    flags = ["--margIsoIncrem", str(K), "--nMassRatios", str(Q)]
    r = _cli("starIntervals", "--config", y, *flags)
    assert r.returncode == 0, r.stderr
    assert "passes" in r.stderr

    cl_f = tm._read_phot(base + ".phot")
    for k in ("obs", "sigma"):                           # (the reference indexes them [star][filter])
        cl_f[k] = cl_f[k].reshape(130, -1)
    got_rows = hostlib.read_res_rows(base + ".res", truth, 3)
    assert np.array_equal(got_rows[:, :9], rows[:, :9]) and len(got_rows) == 34
    eng = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cl_f), priors, tm.opts(1, K, Q))
    try:
        res = hostlib.star_intervals(eng, got_rows)
        res2 = hostlib.star_intervals(eng, got_rows, abi.HQ_SYSTEM, (0.1, 0.9), 1e-3, 4)
    finally:
        eng.close()
    ids, cols, tab = hostlib.read_star_intervals(base + ".starIntervals")
    want = hostlib.star_intervals_table(res)
    assert ids == [str(i + 1) for i in range(130)]
    assert cols == ["member"] + [f"q{a:.12g}{s}" for a in hostlib.STAR_INTERVALS_LEVELS for s in ("", "_lo", "_hi")] + ["passes", "flags"]
    assert tab.shape == want.shape == (130, 18) and np.array_equal(tab, want, equal_nan=True)
    has = ~np.isnan(want[:, 1])
    assert has.sum() >= 110 and np.all(want[has, 17] == 0) and np.all(want[has, 16] <= 12)
    # ... and hold their levels of the reference CDF (the catalogue as the file states it: the field's magnitude ranges are the file's)
    nodes_f = hr.nodes_of_rows(pack_d, cl_f, got_rows, 1, K, Q)
    sc.assert_brackets(cl_f, nodes_f, abi.HQ_PRIMARY, hostlib.STAR_INTERVALS_LEVELS, tab[:, 2:17:3], tab[:, 3:17:3], label="the file")

    r = _cli("starIntervals", "--config", y, *flags, "--quantity", "system", "--levels", "0.1,0.9", "--tol", "1e-3", "--maxPasses", "4")
    assert r.returncode == 0, r.stderr
    _, cols2, tab2 = hostlib.read_star_intervals(base + ".starIntervals")
    assert cols2 == ["member", "q0.1", "q0.1_lo", "q0.1_hi", "q0.9", "q0.9_lo", "q0.9_hi", "passes", "flags"]
    assert np.array_equal(tab2, hostlib.star_intervals_table(res2), equal_nan=True)
    assert np.all(tab2[:, 7] <= 4)
