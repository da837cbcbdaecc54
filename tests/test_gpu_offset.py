"""b9_star_offset (the starOffsets counterpart) on the GPU: star_off and row_off against the numpy statement
tests/offset_ref.py with one and with four directions, with the pruning and without it, with and without a field alternative;
every filter-width instance and both direction tilings; an unused filter, stars a direction does not touch, WD-stage stars, a
row outside the grid; the 32-row chunk; the bit-for-bit ties and invariances; one ragged script; and the CLI.  Each test makes
its own short-lived engine on the small packs of build_problem(small=True); a case's reference is computed once and shared.

Tolerances: tests/offset_check.py (rtol 1e-9 + the pruning's bound per column + the cancellation term of the first moments;
for the log Bayes factor 1e-9 p max(1, |L|, |L'|) + the pruning's bound; with b9_tuning.marg_no_pruning the pruning's bound is
dropped)."""
import functools

import numpy as np
import pytest

import offset_check as oc
import offset_ref as of
import moments_ref as mr
import test_gpu_moments as tm
from base_amd import abi, synth
from conftest import build_problem

pytestmark = pytest.mark.gpu

K = Q = 2
TAU = 0.1


def make_engine(pack, stars, priors, n_pops, K=K, Q=Q):
    from base_amd import engine
    return engine.Engine(pack, stars, priors, tm.opts(n_pops, K, Q))


def four_directions(pack_d):
    """absorption, distance, the first band alone, and an explicit list (a colour term: falling from +1 to -0.5 over the bands)"""
    nf = pack_d["n_filt"]
    return of.directions(pack_d, ["absorption", "distance", "filter:0", np.linspace(1.0, -0.5, nf)])


def compare(got_star, got_rows, ref, cl, ks, taus, n_nodes, pruning=True, cols=None):
    """Both outputs against a reference (star_off, row_off, x, bound, absx); cols: the directions of the reference the call held."""
    want_star, want_rows, x, bound, absx = ref
    C, V = of.all_cv(cl, ks, taus)
    a_star, a_rows = oc.star_atol(bound, absx, n_nodes, pruning), oc.row_atol(bound, absx, C, V, n_nodes, pruning)
    if cols is not None:
        sc = np.r_[0, 1, np.concatenate([np.arange(2 + 3 * j, 5 + 3 * j) for j in cols])]
        rc = np.r_[0, np.concatenate([np.arange(1 + 4 * j, 5 + 4 * j) for j in cols])]
        want_star, a_star, want_rows, a_rows = want_star[:, sc], a_star[:, sc], want_rows[:, rc], a_rows[:, rc]
    print(f"largest relative difference among the entries above 1e-6 ({'pruned' if pruning else 'unpruned'}): star_off "
          f"{oc.largest_rel(got_star, want_star):.3g}, row_off {oc.largest_rel(got_rows, want_rows):.3g}")
    oc.assert_star_off(got_star, want_star, a_star)
    oc.assert_row_off(got_rows, want_rows, a_rows)


def against_reference(pack_d, cl, pack, stars, priors, n_pops, rows, ks, taus, ref=None, nodes=None, subsets=(), K=K, Q=Q):
    """The call with all of ks, then with each subset of them, with the pruning and without it; returns the pruned (star, rows)."""
    n_nodes = tm.n_nodes_of(pack_d, n_pops, K, Q)
    ref = ref or of.reference(pack_d, cl, rows, n_pops, K, Q, ks, taus, nodes)
    taus = np.asarray(taus, dtype=np.float64)
    eng = make_engine(pack, stars, priors, n_pops, K, Q)
    try:
        out = None
        for cols in (None,) + tuple(subsets):
            sel = np.arange(len(ks)) if cols is None else np.asarray(cols)
            for pruning in (True, False):
                eng.set_tuning(**({} if pruning else {"marg_no_pruning": 1}))
                got = eng.star_offset(rows, ks[sel], taus[sel])
                compare(got[0], got[1], ref, cl, ks, taus, n_nodes, pruning, cols)
                out = out or got
            eng.set_tuning()
    finally:
        eng.close()
    return out


@functools.lru_cache(maxsize=None)
def fixture(name, members=False):
    """A non-vacuity fixture of test_offset_host (parsec 4 / dsed 5, 70 stars, WD-stage among them) with test_gpu_moments.rows_for's
    rows (3 + one outside the grid), four directions and their reference.  members: every membership prior 1, so that the
    promoted outliers carry their full weight."""
    args, kw, n_pops = {"parsec4": (("parsec", 4), dict(n_stars=70, wd_frac=0.1, seed=12), 1),
                        "dsed5": (("dsed", 5), dict(n_stars=70, wd_frac=0.1, n_y=3, n_pops=2, seed=12), 2)}[name]
    pack_d, cl, pack, stars, priors, _ = build_problem(*args, **kw)
    if members:
        cl = tm.subset(cl, np.arange(70))
        cl["clust_prior"] = np.ones(70)
        stars = abi.make_stars(cl)
    rows = tm.rows_for(pack_d, cl, n_pops)
    rows.setflags(write=False)
    ks, taus = four_directions(pack_d), [TAU, TAU, 0.2, 0.05]
    nodes = [mr.star_nodes(pack_d, cl, par, n_pops, K, Q) for par in rows]
    return pack_d, cl, pack, stars, priors, n_pops, rows, ks, taus, nodes, of.reference(pack_d, cl, rows, n_pops, K, Q, ks, taus, nodes)


# ---- 1. parity with the reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("members", [False, True], ids=["field", "members"])
@pytest.mark.parametrize("name", ["parsec4", "dsed5"])
def test_parity_with_reference(name, members):
    """D = 4 and D = 1 (each direction alone would do: absorption and the explicit list), pruned and unpruned.  The fixtures hold
    WD-stage stars and a row outside the grid; with every membership prior 1 the stars whose largest boosted term lies thousands
    of e-folds above their largest full term carry their full weight."""
    pack_d, cl, pack, stars, priors, n_pops, rows, ks, taus, nodes, ref = fixture(name, members)
    nv = of.non_vacuity(pack_d, cl, rows[0], n_pops, K, Q, ks[0], taus[0], nodes[0])
    assert nv["shifted"] >= 60 and nv["promoted"] >= 3 and nv["revived"] >= 500
    got_star, got_rows = against_reference(pack_d, cl, pack, stars, priors, n_pops, rows, ks, taus, ref, subsets=((0,), (3,)))
    assert got_star.shape == (70, 14) and got_rows.shape == (4, 17)
    assert np.all(got_rows[-1] == 0) and np.all(got_star[got_star[:, 0] > 0, 0] == 3)      # the row outside the grid adds nothing
    wd = np.asarray(cl["stage"]) == abi.STAGE_WD
    assert (got_star[wd, 1] > 0).sum() >= 3 and np.all(got_star[wd][got_star[wd, 1] > 0][:, 4] != 0)
    if members:
        assert (got_star[:, 1] == 3.0).sum() >= 60


# ---- 2. every filter width, both direction tilings ------------------------------------------------------------------------
@pytest.mark.parametrize("n_filt,n_pops,n_dir", [(8, 1, 3), (8, 2, 2), (9, 1, 1), (9, 2, 3), (16, 1, 4), (16, 2, 3), (4, 2, 4), (1, 1, 2)])
def test_every_instance(n_filt, n_pops, n_dir):
    """8 filters, and 9 and 16 in the 16-filter instances (which hold two directions a tile: 3 and 4 directions run two tiles,
    the second half empty at 3); three directions at 4 or 8 filters run the four-direction instance with one idle."""
    pack_d, cl, pack, stars, priors, _ = build_problem("dsed" if n_pops == 2 else "parsec", n_filt, n_stars=70, wd_frac=0.1,
                                                       n_y=3 if n_pops == 2 else 1, n_pops=n_pops, seed=12)
    rows = tm.rows_for(pack_d, cl, n_pops, 2, outside=False)
    ks, taus = four_directions(pack_d)[:n_dir], [TAU, 0.3, 0.2, 0.05][:n_dir]
    got_star, got_rows = against_reference(pack_d, cl, pack, stars, priors, n_pops, rows, ks, taus)
    assert got_star.shape[1] == 2 + 3 * n_dir and got_rows.shape[1] == 1 + 4 * n_dir and (got_star[:, 1] > 0).sum() >= 40


# ---- 3. edge cases ----------------------------------------------------------------------------------------------------------
def test_special_stars():
    """An MS/RGB and a WD-stage star with one filter unused each, direction filter:<that band> among the directions: C = 0, the
    three columns are exact zeros and the star is absent from that direction's row sums (shown on one row by re-adding them in
    the kernel's order); a star with every filter unused (C = 0 in every direction); membership priors of 1e-300 and 1."""
    pack_d, cl, pack, _, priors, _ = build_problem("parsec", 4, n_stars=70, wd_frac=0.1, seed=12)
    cl = tm.subset(cl, np.arange(70))
    cl["sigma"] = np.array(cl["sigma"], dtype=np.float64)
    cl["clust_prior"] = np.array(cl["clust_prior"], dtype=np.float64)
    ms = np.flatnonzero((np.asarray(cl["stage"]) != abi.STAGE_WD) & (cl["sigma"] > 0).all(axis=1))
    wd = np.flatnonzero((np.asarray(cl["stage"]) == abi.STAGE_WD) & (cl["sigma"] > 0).all(axis=1))
    cl["sigma"][ms[3]] = -1.0
    cl["clust_prior"][ms[5]] = 1e-300
    cl["clust_prior"][ms[7]] = 1.0
    cl["sigma"][ms[9], 2] = -1.0
    cl["sigma"][wd[0], 2] = -1.0
    rows = tm.rows_for(pack_d, cl, 1)
    stars = abi.make_stars(cl)
    ks, taus = of.directions(pack_d, ["absorption", "filter:2", "distance"]), [TAU, 0.2, TAU]
    got, got_rows = against_reference(pack_d, cl, pack, stars, priors, 1, rows, ks, taus)
    assert got[wd[0], 1] > 0 and got[ms[9], 1] > 0
    assert got[ms[5], 0] == 3 and np.all(np.abs(got[ms[5], 1:]) < 1e-250)
    assert got[ms[7], 1] == 3.0
    assert got[ms[3], 0] == 3 and got[ms[3], 1] > 0 and np.all(got[ms[3], 2:] == 0)
    for i in (ms[9], wd[0]):
        assert np.all(got[i, 5:8] == 0) and np.all(got[i, 2:5] != 0) and np.all(got[i, 8:11] != 0)
    eng = make_engine(pack, stars, priors, 1)
    try:
        x, rws = eng.star_offset(rows[:1], ks, taus)
    finally:
        eng.close()
    C, V = of.all_cv(cl, ks, taus)
    for j in range(3):
        a = np.zeros(4)
        for i in range(70):
            if C[i, j] > 0:
                a = a + np.array([x[i, 1], x[i, 2 + 3 * j], x[i, 3 + 3 * j] + x[i, 1] * V[i, j], x[i, 4 + 3 * j]])
        assert np.array_equal(rws[0, [1 + 4 * j, 2 + 4 * j, 4 + 4 * j]], a[[0, 1, 3]])
        assert abs(rws[0, 3 + 4 * j] - a[2]) <= 1e-13 * a[2]                 # (V_i is the device's: an ulp from numpy's)
    assert rws[0, 1 + 4 * 1] < rws[0, 1 + 4 * 0] and rws[0, 1] < rws[0, 0]


# ---- 4. chunking ------------------------------------------------------------------------------------------------------------
def test_chunk_seam_against_reference():
    """33 rows: one call is a chunk of 32 and a chunk of 1."""
    pack_d, cl, pack, stars, priors, _ = build_problem("parsec", 4, n_stars=70, wd_frac=0.1, seed=12)
    rows = synth.walker_params(cl["truth"], 33, seed=8, scale=0.3)
    ks, taus = of.directions(pack_d, ["absorption", "distance"]), [TAU, TAU]
    ref = of.reference(pack_d, cl, rows, 1, K, Q, ks, taus)
    eng = make_engine(pack, stars, priors, 1)
    try:
        star, rws = eng.star_offset(rows, ks, taus)
        compare(star, rws, ref, cl, ks, taus, tm.n_nodes_of(pack_d, 1, K, Q))
        last, last_row = eng.star_offset(rows[32:], ks, taus)
    finally:
        eng.close()
    assert (star[:, 0] == 33).sum() >= 60 and np.array_equal(rws[32], last_row[0])


# ---- 5. bitwise ties and invariances ----------------------------------------------------------------------------------------
def test_bitwise_invariances():
    pack_d, cl, pack, stars, priors, n_pops, _, ks, taus, _, _ = fixture("dsed5")
    taus = np.asarray(taus)
    rows = synth.walker_params(cl["truth"], 40, seed=8, scale=0.3, n_pops=2)
    rows[:, abi.P_LAMBDA] = np.clip(rows[:, abi.P_LAMBDA], 0.05, 0.95)
    edges = np.linspace(0.1, 8.0, 25)
    eng = make_engine(pack, stars, priors, n_pops)
    try:
        whole, whole_rows = eng.star_offset(rows, ks, taus)
        assert (whole[:, 0] == 40).sum() >= 60
        # x[0] and x[1] are b9_phot_resid's bits
        res, _ = eng.phot_resid(rows)
        assert np.array_equal(whole[:, :2], res[:, :2])
        # one call = the same call split by B9_OFF_CONTINUE at rows 1, 16 and 32
        acc, parts = None, []
        for lo, hi in ((0, 1), (1, 16), (16, 32), (32, 40)):
            acc, r = eng.star_offset(rows[lo:hi], ks, taus, acc)
            parts.append(r)
        assert np.array_equal(acc, whole) and np.array_equal(np.concatenate(parts), whole_rows)
        # either output NULL
        only_star, none = eng.star_offset(rows, ks, taus, want_rows=False)
        assert none is None and np.array_equal(only_star, whole)
        none, only_rows = eng.star_offset(rows, ks, taus, want_star=False)
        assert none is None and np.array_equal(only_rows, whole_rows)
        # a direction alone (and a pair) equals the same direction among four
        for sel in ([0], [1], [2], [3], [1, 3], [3, 0, 2]):
            s, r = eng.star_offset(rows, ks[sel], taus[sel])
            for q, j in enumerate(sel):
                assert np.array_equal(s[:, 2 + 3 * q:5 + 3 * q], whole[:, 2 + 3 * j:5 + 3 * j]), sel
                assert np.array_equal(r[:, 1 + 4 * q:5 + 4 * q], whole_rows[:, 1 + 4 * j:5 + 4 * j]), sel
            assert np.array_equal(s[:, :2], whole[:, :2]) and np.array_equal(r[:, 0], whole_rows[:, 0])
        # k -> 2 k with tau -> tau / 2: the means halve, the second moments quarter, the log Bayes factors keep their bits
        s2, r2 = eng.star_offset(rows, 2.0 * ks, 0.5 * taus)
        assert np.array_equal(s2[:, :2], whole[:, :2])
        assert np.array_equal(s2[:, 2::3], 0.5 * whole[:, 2::3]) and np.array_equal(s2[:, 3::3], 0.25 * whole[:, 3::3])
        assert np.array_equal(s2[:, 4::3], whole[:, 4::3])
        assert np.array_equal(r2[:, 2::4], 0.5 * whole_rows[:, 2::4]) and np.array_equal(r2[:, 3::4], 0.25 * whole_rows[:, 3::4])
        assert np.array_equal(r2[:, 4::4], whole_rows[:, 4::4]) and np.array_equal(r2[:, 1::4], whole_rows[:, 1::4])
        # a repeated call; other chain calls in between leave nothing behind
        eng.mass_hist(rows[:5], edges, abi.HQ_SYSTEM)
        eng.filter_loo(rows[:3])
        eng.star_offset(rows[:2], ks[:1], taus[:1])
        again, again_rows = eng.star_offset(rows, ks, taus)
        assert np.array_equal(again, whole) and np.array_equal(again_rows, whole_rows)
    finally:
        eng.close()
    eng = make_engine(pack, stars, priors, n_pops)                             # a fresh context
    try:
        fresh, fresh_rows = eng.star_offset(rows, ks, taus)
        assert np.array_equal(fresh, whole) and np.array_equal(fresh_rows, whole_rows)
    finally:
        eng.close()
    # a star's line does not depend on the other stars of the catalogue: each star alone, and every third star together
    for keep in [np.array([i]) for i in (0, 1, 17, 42, 69)] + [np.arange(0, 70, 3)]:
        eng = make_engine(pack, abi.make_stars(tm.subset(cl, keep)), priors, n_pops)
        try:
            part, _ = eng.star_offset(rows, ks, taus)
        finally:
            eng.close()
        assert np.array_equal(part, whole[keep]), keep
    wd = np.flatnonzero(np.asarray(cl["stage"]) == abi.STAGE_WD)
    eng = make_engine(pack, abi.make_stars(tm.subset(cl, wd[:1])), priors, n_pops)        # a WD-stage star alone
    try:
        part, _ = eng.star_offset(rows, ks, taus)
    finally:
        eng.close()
    assert np.array_equal(part, whole[wd[:1]]) and part[0, 1] > 0


def test_errors_leave_the_outputs_untouched():
    import ctypes as C
    _dp = C.POINTER(C.c_double)
    pack_d, cl, pack, stars, priors, n_pops, rows, ks, taus, _, _ = fixture("parsec4")
    rows, ks, taus = np.ascontiguousarray(rows), np.ascontiguousarray(ks[:2]), np.ascontiguousarray(taus[:2], dtype=np.float64)
    eng = make_engine(pack, stars, priors, n_pops)
    try:
        def call(n_rows=4, n_dir=2, star=True, rws=True, k=ks, tau=taus):
            so, ro = np.full((70, 2 + 3 * 4), 7.25), np.full((4, 1 + 4 * 4), 7.25)
            p = lambda a: a.ctypes.data_as(_dp) if a is not None else None      # noqa: E731
            code = eng.lib.b9_star_offset(eng._ctx, p(rows), n_rows, 0, n_dir, p(k), p(tau), p(so) if star else None, p(ro) if rws else None)
            assert code == abi.B9_OK or (np.all(so == 7.25) and np.all(ro == 7.25))
            return code

        assert call() == abi.B9_OK and call(star=False) == abi.B9_OK and call(rws=False) == abi.B9_OK
        assert call(n_rows=0) == abi.B9_ERR_INVALID and call(star=False, rws=False) == abi.B9_ERR_INVALID
        assert call(n_dir=0) == abi.B9_ERR_INVALID and call(n_dir=5) == abi.B9_ERR_INVALID
        assert call(k=None) == abi.B9_ERR_INVALID and call(tau=None) == abi.B9_ERR_INVALID
        assert call(tau=np.array([0.1, 0.0])) == abi.B9_ERR_INVALID and call(tau=np.array([0.1, np.inf])) == abi.B9_ERR_INVALID
        bad = ks.copy(); bad[1, 2] = np.nan
        assert call(k=bad) == abi.B9_ERR_INVALID
    finally:
        eng.close()


# ---- 6. one ragged script ---------------------------------------------------------------------------------------------------
def test_ragged_script():
    """Script 4 of tests/ragged_chain.py (140 stars, 25 WD-stage; 36 rows whose tables run from 158 points to 2, vanish -- no
    isochrone, a row outside the grid -- and come back, the 32-row seam between a vanished table and the longest) against the
    reference, and every row's increment against the row alone on a context that has done nothing else."""
    import ragged_chain as rcn
    combo = ("base4", 2, 2)
    ref = rcn.reference(*combo)
    prob = ref.prob
    rows = prob["scripts"][4]
    facts = [rcn.row_facts(prob["pack_d"], r, combo[1], prob["n_pops"])[0] for r in rows]
    assert facts[31] != "valid" and facts[32] == "valid" and sum(f != "valid" for f in facts) >= 4
    pack_d, cl = prob["pack_d"], prob["cl"]
    ks, taus = of.directions(pack_d, ["absorption", "distance"]), [TAU, TAU]
    want = of.reference(pack_d, cl, rows, prob["n_pops"], combo[1], combo[2], ks, taus, ref.nodes(rows))
    from base_amd import engine
    eng = engine.Engine(*rcn.device_args(prob, combo[1], combo[2]))
    try:
        for pruning in (True, False):
            eng.set_tuning(**({} if pruning else {"marg_no_pruning": 1}))
            star, rws = eng.star_offset(rows, ks, taus)
            compare(star, rws, want, cl, ks, taus, ref.n_nodes, pruning)
        eng.set_tuning()
        steps = [eng.star_offset(rows[:j + 1], ks, taus) for j in range(len(rows))]
    finally:
        eng.close()
    alone = {}
    for j, r in enumerate(rows):
        if r.tobytes() not in alone:
            e = engine.Engine(*rcn.device_args(prob, combo[1], combo[2]))
            try:
                alone[r.tobytes()] = e.star_offset(r[None, :], ks, taus)
            finally:
                e.close()
        one, one_row = alone[r.tobytes()]
        before = steps[j - 1][0] if j else np.zeros_like(one)
        assert np.array_equal(steps[j][0], before + one), j
        assert np.array_equal(steps[j][1][j], one_row[0]) and np.array_equal(steps[-1][1][j], one_row[0]), j
    assert len(alone) < len(rows) and any(np.all(a[0] == 0) for a in alone.values())


# ---- 7. the CLI -------------------------------------------------------------------------------------------------------------
def test_cli_star_offsets(tmp_path):
    """simCluster (70 stars) -> scatterCluster -> singlePopMcmc (short, 4 walkers x 70 main-run rows: the program passes them in
    two batches, the second continued) -> starOffsets with three directions: both files read back to the bits of what
    Engine.star_offset in ONE call gives through hostlib.offset_table / offset_dist_table."""
    from base_amd import build, engine, host_build, hostlib
    from cli_util import cli as _cli
    build.build_hip()
    host_build.build_host()
    pack_d = synth.make_pack("parsec", 8, n_feh=4, n_age=8, n_eep=90)
    truth = synth.default_params(pack_d)
    truth[abi.P_IFMR_INTERCEPT], truth[abi.P_IFMR_SLOPE], truth[abi.P_IFMR_QUAD] = 0.77, 0.08, 0.0   # the session's defaults
    root = synth.write_models_dir(pack_d, str(tmp_path / "models"))
    base = str(tmp_path / "run")
    y_true = synth.write_yaml(str(tmp_path / "truth.yaml"), base + ".sim.scatter", root, base, truth, seed=17)
    r = _cli("simCluster", "--config", y_true, "--nStars", "70", "--percentBinary", "30", "--minMass", "0.4")
    assert r.returncode == 0, r.stderr
    r = _cli("scatterCluster", "--config", y_true, "--sigmaFloor", "0.01", "--sigmaAtLimit", "0.05", "--faintLimit", "45")
    assert r.returncode == 0, r.stderr
    start = truth.copy()
    start[abi.P_LOGAGE] += 0.004; start[abi.P_MOD] += 0.01; start[abi.P_FEH] -= 0.01
    fit = str(tmp_path / "fit")
    y = synth.write_yaml(str(tmp_path / "fit.yaml"), base + ".sim.scatter", root, fit, start, burn=200, run=70, walkers=4)
    r = _cli("singlePopMcmc", "--config", y, "--priorFe_H", repr(float(truth[abi.P_FEH])), "--priorDistMod", repr(float(truth[abi.P_MOD])),
             "--priorAv", repr(float(truth[abi.P_ABS])))
    assert r.returncode == 0, r.stderr
    cl = tm._read_phot(base + ".sim.scatter")
    header = open(base + ".sim.scatter").read().splitlines()[0].split()
    filters = header[1:1 + cl["n_filt"]]
    specs = ["absorption", "distance", "filter:" + filters[2]]
    r = _cli("starOffsets", "--config", y, "--direction", specs[0], "--direction", specs[1], "--direction", specs[2], "--tau", "0.1", "--tau", "0.1",
             "--tau", "0.25")
    assert r.returncode == 0, r.stderr
    assert "star rows/s" in r.stderr

    phot_ids = [ln.split()[0] for ln in open(base + ".sim.scatter").read().splitlines()[1:]]
    rows = hostlib.read_res_rows(fit + ".res", start, 3)
    assert len(rows) == 70 * 4                            # more than one batch of 256
    sigma = cl["sigma"].reshape(-1, cl["n_filt"])
    ks, taus = hostlib.offset_directions(specs, filters, pack_d["abs_coeff"]), [0.1, 0.1, 0.25]
    assert np.array_equal(ks, of.directions(pack_d, ["absorption", "distance", "filter:2"]))
    eng = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cl), synth.default_priors(pack_d, truth), tm.opts(1, 4, 4))      # the program's default grid
    try:
        star, rws = eng.star_offset(rows, ks, taus)
    finally:
        eng.close()
    ids, cols, tab = hostlib.read_star_offsets(fit + ".starOffsets")
    assert ids == phot_ids and cols == ["rows", "member"] + [f"{d}_{c}" for d in specs for c in hostlib.OFFSET_STAR_COLUMNS]
    assert np.array_equal(tab, hostlib.offset_table(star, sigma, ks, taus))
    assert np.all(tab[:, 0] == len(rows)) and (tab[:, 1] > 0.9).sum() >= 35
    names, cols, dtab = hostlib.read_offset_dist(fit + ".offsetDist")
    assert names == specs and cols == list(hostlib.OFFSET_DIST_COLUMNS)
    assert np.array_equal(dtab, hostlib.offset_dist_table(rws, 3))
    members = tab[:, 1] > 0.9
    print(f"{members.sum()} members: |z| of the absorption offset at most {np.abs(tab[members, 4]).max():.3g}, mean logBF {tab[members, 5].mean():.3g}")
    assert np.all(dtab[:, 0] == len(rows)) and np.all(tab[members, 3] > 0)
