"""The host side of wdIntervals without a GPU: the comparator of tests/wdbins_check.py rejects every mutation of the numpy
statement of b9_wd_bins (tests/wdbins_ref.py), the parity fixtures' conditions hold, the generalised refinement loop driven by
that statement ends with brackets that hold their levels, hostlib.star_intervals gives the parent commit's results bit for bit,
and the table, the file and the settings of the program."""
import os

import numpy as np
import pytest

import masshist_ref as hr
import starbins_ref as sr
import wdbins_check as bc
import wdbins_ref as br
import wdmoments_check as wc
import wdmoments_ref as wr
from base_amd import abi, hostlib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "recorded", "starintervals_parent.npz")


class NumpyWdEngine:
    """What hostlib.wd_intervals needs of an engine, from the numpy statements: wd_moments and wd_bins over the rows' lines."""

    def __init__(self, pack_d, cl, n_pops):
        self.pack_d, self.cl, self.n_pops = pack_d, cl, n_pops
        self.calls, self.lines = 0, {}

    def _lines(self, rows, n_nodes):
        key = (rows.tobytes(), n_nodes)
        if key not in self.lines:
            self.lines[key] = [br.row_lines(self.pack_d, self.cl, par, self.n_pops, n_nodes) for par in rows]
        return self.lines[key]

    def wd_moments(self, rows, n_nodes, acc=None):
        return wr.accumulate(self.pack_d, self.cl, rows, self.n_pops, n_nodes), wr.wd_stars(self.cl)

    def wd_bins(self, rows, n_nodes, edges, quantities=br.ALL, acc=None):
        self.calls += 1
        n_wd = len(wr.wd_stars(self.cl))
        return bc.summed(bc.reference_rows(self._lines(rows, n_nodes), n_wd, quantities, edges)), wr.wd_stars(self.cl)


# ---- 1. the comparator rejects every mutation ------------------------------------------------------------------------------------
def test_comparator_rejects_every_mutation():
    pack_d, cl, priors, rows, n_pops, n_nodes = wc.parity_fixture("girardi")[:6]
    lines, edges, _, _ = bc.parity_lines("girardi")
    n_wd = len(wr.wd_stars(cl))
    for n_bins in (1, 2, 30):
        e = bc.sub_edges(edges, n_bins)
        x = bc.reference_rows(lines, n_wd, br.ALL, e)
        bc.assert_close(bc.summed(x), br.accumulate(pack_d, cl, rows, n_pops, n_nodes, br.ALL, e), "the reference against itself")
        for mutation in ("closed_right", "other_line_edges"):
            # closed on the right differs only for a value ON an edge: the edges are moved onto node values for it
            ee = e
            if mutation == "closed_right":
                ee = e.copy()
                for c in range(n_wd):
                    for s in range(6):
                        v, m, _ = br.line_mixture(lines, rows, c, s)
                        heavy = np.unique(v[m > 1e-3 * m.sum()]) if len(v) else v
                        if len(heavy) >= n_bins + 1:
                            ee[c, s] = heavy[np.round(np.linspace(0, len(heavy) - 1, n_bins + 1)).astype(int)]
                assert np.all(np.diff(ee, axis=2) > 0)
            want = bc.summed(bc.reference_rows(lines, n_wd, br.ALL, ee))
            wrong = bc.summed(np.stack([br.increments_of(ln, n_wd, br.ALL, ee, **{mutation: True}) for ln in lines]))
            assert bc.rejects(bc.assert_close, wrong, want), (mutation, n_bins)
    # derived values over all nodes: the seam fixture, where some nodes' precursors are still alive (their derived values are 0)
    pack_d, cl, priors, rows, n_nodes = wc.seam_fixture()
    for n_bins in (1, 2, 30):
        e = np.tile(np.linspace(-1.0, 20.0, n_bins + 1), (6, 6, 1))
        want = br.increments(pack_d, cl, rows[0], 1, n_nodes, br.ALL, e)
        assert bc.rejects(bc.assert_close, br.increments(pack_d, cl, rows[0], 1, n_nodes, br.ALL, e, derived_over_all_nodes=True), want), n_bins
    # the population weight: a two-population fixture
    pack_d, cl, priors, rows, n_pops, n_nodes = wc.parity_fixture("dsed")[:6]
    lines, edges, _, _ = bc.parity_lines("dsed")
    want = bc.reference_rows(lines[:1], 150, br.ALL, edges)[0]
    wrong = br.increments(pack_d, cl, rows[0], n_pops, n_nodes, br.ALL, edges, drop_pop_weight=True)
    assert bc.rejects(bc.assert_close, wrong, want)
    # the total where nothing is cooled: the seam fixture with M_wd_up lowered into its band of precursors that are still alive
    from base_amd import synth
    pack_d, cl, priors, rows, n_nodes = wc.seam_fixture()
    par = rows[0]
    tip = synth.derive_isochrone(pack_d, par[abi.P_LOGAGE], par[abi.P_FEH], par[abi.P_Y])[1][-1]
    pack_d = dict(pack_d, m_wd_up=tip + 4.5 * (pack_d["m_wd_up"] - tip) / n_nodes)
    e = np.tile(np.linspace(-1.0, 20.0, 4), (6, 6, 1))
    want = br.increments(pack_d, cl, par, 1, n_nodes, br.ALL, e)
    assert np.all(want[:, 1:, :5] == 0) and (want[:, 1:, 5] > 0).all() and np.array_equal(want[:, 1, 5], want[:, 0, 5])
    assert bc.rejects(bc.assert_close, br.increments(pack_d, cl, par, 1, n_nodes, br.ALL, e, drop_total_uncooled=True), want)


# ---- 2. the parity fixtures' conditions, from the reference alone ---------------------------------------------------------------
@pytest.mark.parametrize("key", ["girardi", "dsed", "parsec"])
def test_parity_fixture_conditions(key):
    lines, edges, replaced, margin = bc.parity_lines(key)
    x = bc.summed(bc.reference_rows(lines, 150, br.ALL, edges))
    inner, C = bc.inner_bins_with_mass(x)
    has = C > 0
    print(f"{key}: {int((inner[has] >= 3).sum())} of {int(has.sum())} lines with >= 3 inner bins above 1e-3; smallest margin "
          f"{margin[has].min():.3g} tolerances; replaced edges per quantity {replaced.sum(axis=0)}")
    assert edges.shape == (150, 6, 31) and np.all(np.diff(edges, axis=2) > 0)
    assert np.all(margin >= bc.MARGIN)
    assert has.sum() >= 6 * 100 and (inner[has] >= 3).sum() >= 0.9 * has.sum()


# ---- 3. the generalised loop on the reference --------------------------------------------------------------------------------------
def test_wd_intervals_on_the_reference():
    """4 WD-stage stars x 5 quantities = 20 lines, 6 rows, 64 nodes: the loop, started on the ranges the moments give, ends with
    brackets that contain the reference CDF's levels."""
    pack_d, cl, priors = wc.wd_problem("parsec", 8, 400, keep=4)
    rows = wc.rows_for(cl, 6, 3, 1)
    mask = br.ALL & ~(1 << 2)
    eng = NumpyWdEngine(pack_d, cl, 1)
    res = hostlib.wd_intervals(eng, rows, 64, mask)
    assert res["n_wd"] == 4 and res["n_sel"] == 5 and res["value"].shape == (20, 5) and res["n_passes"] == eng.calls <= 12
    lo, hi = hostlib.wd_first_ranges(eng.wd_moments(rows, 64)[0], mask)
    assert np.array_equal(lo, res["first_lo"]) and np.array_equal(hi, res["first_hi"]) and np.all(hi > lo)
    lines = eng._lines(rows, 64)
    has = bc.assert_brackets(lines, rows, 4, mask, res["levels"], res["lo"], res["hi"], res["final"], 1e-4, "20 lines")
    good = has & res["final"].all(axis=1)
    print(f"{int(good.sum())} of {int(has.sum())} lines final after {res['n_passes']} passes; passes used {np.bincount(res['passes'])}")
    assert has.sum() >= 15 and good.sum() >= 0.9 * has.sum()
    assert np.all(res["flags"][~has] == hostlib.SIV_NO_MASS) and np.isnan(res["value"][~has]).all()
    assert np.all((res["value"][has] >= res["lo"][has]) & (res["value"][has] <= res["hi"][has]))
    # counted: 1 for the ZAMS mass, the cooled share for the derived quantities
    wd_acc = eng.wd_moments(rows, 64)[0]
    counted = res["counted"].reshape(4, 5)
    np.testing.assert_allclose(counted[:, 0], 1.0, rtol=1e-12)
    np.testing.assert_allclose(counted[:, 1:], np.repeat((wd_acc[:, wr.COOLED] / wd_acc[:, wr.MEMBER])[:, None], 4, axis=1), rtol=1e-9)
    # the first ranges: mean -/+ max(6 sd, 1e-3 |mean|) of the table's columns; [0, 1] without counted mass
    tab = wr.table(wd_acc)
    mean, sd = tab[:, [3, 5, 9, 11, 13]], tab[:, [4, 6, 10, 12, 14]]
    half = np.maximum(6 * sd, 1e-3 * np.abs(mean))
    np.testing.assert_allclose(lo, mean - half, rtol=1e-12)
    np.testing.assert_allclose(hi, mean + half, rtol=1e-12)
    z_lo, z_hi = hostlib.wd_first_ranges(np.zeros((2, 16)), br.ALL)
    assert np.all(z_lo == 0) and np.all(z_hi == 1) and z_lo.shape == (2, 6)


# ---- 4. star_intervals is the loop on [0, 2 max_mass]: the parent commit's results, bit for bit -------------------------------
def test_star_intervals_gives_the_recorded_results():
    """tests/test_starbins_host.py's case through hostlib.star_intervals, against its inputs and outputs recorded at the commit
    before the loop was factored out."""
    import test_starbins_host as ts
    pack_d, cl, rows, nodes, max_mass = ts.case()
    g = np.load(GOLDEN)
    assert np.array_equal(g["rows"], rows) and float(g["max_mass"]) == max_mass
    e0 = np.tile(2.0 * max_mass * (np.arange(31) / 30.0), (60, 1))
    for q, name in ((hr.PRIMARY, "primary"), (hr.SYSTEM, "system")):
        eng = sr.NumpyEngine(pack_d, cl, 1, ts.K, ts.Q, nodes, max_mass)
        assert np.array_equal(eng.star_bins(rows, e0, q), g[name + "_first_acc"])           # the inputs are the recorded ones
        res = hostlib.star_intervals(eng, rows, q)
        for k in ("member", "value", "lo", "hi", "final", "passes", "flags", "edges", "acc"):
            assert np.array_equal(np.asarray(res[k]), g[name + "_" + k], equal_nan=True), (name, k)
        assert res["n_passes"] == int(g[name + "_n_passes"])
    res = hostlib.star_intervals(sr.NumpyEngine(pack_d, cl, 1, ts.K, ts.Q, nodes, max_mass), rows, hr.PRIMARY, (0.1, 0.9), 1e-3, 3)
    for k in ("member", "value", "lo", "hi", "final", "passes", "flags", "edges"):
        assert np.array_equal(np.asarray(res[k]), g["short_" + k], equal_nan=True), k
    # ... and it is interval_loop on [0, 2 max_mass]
    eng = sr.NumpyEngine(pack_d, cl, 1, ts.K, ts.Q, nodes, max_mass)
    loop = hostlib.interval_loop(lambda e: eng.star_bins(rows, e, hr.PRIMARY), np.zeros(60), np.full(60, 2.0 * max_mass), 12)
    assert np.array_equal(loop["value"], g["primary_value"], equal_nan=True) and np.array_equal(loop["edges"], g["primary_edges"])


# ---- 5. the table and the file -----------------------------------------------------------------------------------------------------
def test_table_and_file_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    n_wd, mask, levels = 7, (1 << 0) | (1 << 3) | (1 << 5), (0.16, 0.5, 0.84)
    n_sel, m = 3, 3
    res = dict(n_wd=n_wd, n_sel=n_sel, member=np.repeat(rng.random(n_wd), n_sel), counted=rng.random(n_wd * n_sel),
               value=rng.normal(size=(n_wd * n_sel, m)), lo=rng.normal(size=(n_wd * n_sel, m)), hi=rng.normal(size=(n_wd * n_sel, m)),
               passes=rng.integers(1, 12, n_wd * n_sel).astype(np.int32), flags=rng.integers(0, 3, n_wd * n_sel).astype(np.int32))
    res["value"][4] = np.nan; res["lo"][4] = np.nan; res["hi"][4] = np.nan          # a line without counted mass
    res["lo"][5, 0] = -np.inf; res["hi"][6, 2] = np.inf                             # open brackets
    tab = hostlib.wd_intervals_table(res)
    assert tab.shape == (n_wd, 1 + n_sel * (3 * m + 3))
    per = 3 * m + 3
    for i in range(n_wd):
        assert tab[i, 0] == res["member"][i * n_sel]
        for s in range(n_sel):
            t, line = tab[i, 1 + s * per:1 + (s + 1) * per], i * n_sel + s
            assert t[0] == res["counted"][line] and t[-2] == res["passes"][line] and t[-1] == res["flags"][line]
            assert np.array_equal(t[1:-2].reshape(m, 3), np.stack([res["value"][line], res["lo"][line], res["hi"][line]], axis=1), equal_nan=True)
    ids = [f"wd{i}" for i in range(n_wd)]
    path = str(tmp_path / "x.wdIntervals")
    hostlib.write_wd_intervals(path, ids, mask, levels, tab)
    got_ids, cols, got = hostlib.read_wd_intervals(path)
    want_cols = ["member"]
    for n in ("zamsMass", "logCoolAge", "logg"):
        want_cols += [n + "_counted"] + [f"{n}_q{a:.12g}{s}" for a in levels for s in ("", "_lo", "_hi")] + [n + "_passes", n + "_flags"]
    assert got_ids == ids and cols == want_cols and np.array_equal(got, tab, equal_nan=True)
    assert hostlib.wd_quantity_mask(("zamsMass", "logCoolAge", "logg")) == mask
    with pytest.raises(hostlib.HostError):
        hostlib.write_wd_intervals(path, ids, 0, levels, tab[:, :1])


# ---- 6. the program's settings -----------------------------------------------------------------------------------------------------
def test_settings(tmp_path):
    d = hostlib.wd_intervals_settings([])
    assert d == dict(quantities=63, levels=hostlib.STAR_INTERVALS_LEVELS, tol=1e-4, maxPasses=12, nMassNodes=512, nPops=1)
    d = hostlib.wd_intervals_settings(["--quantities", "logg,zamsMass", "--levels", "0.1,0.5,0.9", "--tol", "1e-6", "--maxPasses", "20", "--nPops", "2",
                                       "--nMassNodes", "100"])
    assert d == dict(quantities=(1 << 0) | (1 << 5), levels=(0.1, 0.5, 0.9), tol=1e-6, maxPasses=20, nMassNodes=100, nPops=2)
    y = tmp_path / "s.yaml"
    y.write_text("wdIntervals:\n  quantities: [wdMass, logTeff]\n  levels: [0.25, 0.75]\n  tol: 1e-3\n  maxPasses: 5\n  nPops: 2\n")
    d = hostlib.wd_intervals_settings(["--config", str(y)])
    assert d == dict(quantities=(1 << 1) | (1 << 4), levels=(0.25, 0.75), tol=1e-3, maxPasses=5, nMassNodes=512, nPops=2)
    assert hostlib.wd_intervals_settings(["--config", str(y), "--quantities=logg"])["quantities"] == 1 << 5       # a flag overrides the file
    # the nMassNodes fallback chain: wdIntervals', then wdSummary's, then sampleWDMass's, then 512
    y.write_text("sampleWDMass:\n  nMassNodes: 300\n")
    assert hostlib.wd_intervals_settings(["--config", str(y)])["nMassNodes"] == 300
    y.write_text("sampleWDMass:\n  nMassNodes: 300\nwdSummary:\n  nMassNodes: 200\n")
    assert hostlib.wd_intervals_settings(["--config", str(y)])["nMassNodes"] == 200
    y.write_text("sampleWDMass:\n  nMassNodes: 300\nwdSummary:\n  nMassNodes: 200\nwdIntervals:\n  nMassNodes: 100\n")
    assert hostlib.wd_intervals_settings(["--config", str(y)])["nMassNodes"] == 100
    assert hostlib.wd_intervals_settings(["--config", str(y), "--nMassNodes", "50"])["nMassNodes"] == 50
    for bad in (["--quantities", "zamsMass,mass"], ["--quantities", ""], ["--levels", ",".join(str(x) for x in np.linspace(0.05, 0.95, 11))],
                ["--levels", "0.5,0.4"], ["--tol", "-1"], ["--maxPasses", "0"], ["--nMassNodes", "0"], ["--nPops", "3"], ["--perRow"]):
        with pytest.raises(hostlib.HostError):
            hostlib.wd_intervals_settings(bad)
    # starIntervals keeps its own spellings
    assert hostlib.star_intervals_settings(["--levels", "0.1,0.9"])["levels"] == (0.1, 0.9)
    assert hostlib.wd_intervals_settings(["--levels", "0.1,0.9"])["levels"] == (0.1, 0.9)
