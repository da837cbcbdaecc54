"""GPU tests of b9_cmd_band (Engine.cmd_band, hostlib.cmd_band, the program cmdBand) against tests/band_ref.py through
tests/band_check.py, on the ladder pack of tests/ragged_walk.py: cells of 158, 66 / 65 / 64, 34 / 33 / 32, 3, 2 and 1 common EEPs,
settings base4, wdragged5 (two populations, a helium axis, ragged WD tracks) and base9, 40 scripted rows that hop between the
cells and leave the grid (band_ref.scripted_rows: no WD node on the prec = logAge seam or inside the pack's ambiguous tip band)."""
import ctypes as C
import functools

import numpy as np
import pytest

import band_check as bc
import band_ref as br
import ragged_chain as rch
import ragged_walk as rw
from base_amd import abi, engine, hostlib, synth
from cli_util import cli as _cli

pytestmark = pytest.mark.gpu

_dp = C.POINTER(C.c_double)
NODES = rch.WD_NODES                                     # 63 and 65
LEVELS = (0.0313, 0.1687, 0.5171, 0.8329, 0.9771)           # a N is no integer for any N below 10000
#: the spec variations: ratios {0, 0.5, 1}, both node counts, both atmosphere types, two colours, the whole EEP range and a window
SPECS = {
    "wide": br.spec_of(0, 160, (0.0, 0.5, 1.0), NODES[0], 3, ((0, 1), (2, 1))),
    "window": br.spec_of(10, 60, (1.0, 0.0), NODES[1], 2, ((3, 0),)),
}


@functools.lru_cache(maxsize=None)
def problem(setting, dark=False):
    s = rch.SETTINGS[setting]
    pack_d = rw.ladder_pack(s.n_filt, s.n_y, rch.PACK_SEED, s.variant)
    if dark:
        pack_d = br.dark_pack(pack_d)
    rows = br.scripted_rows(pack_d, s.n_pops, NODES)
    return dict(setting=s, pack_d=pack_d, pack=abi.make_pack(pack_d), rows=rows, n_pops=s.n_pops, n_filt=s.n_filt)


@functools.lru_cache(maxsize=None)
def reference(setting, spec_name, dark=False):
    p = problem(setting, dark)
    vals = br.values(p["pack_d"], p["rows"], p["n_pops"], SPECS[spec_name])
    vals.setflags(write=False)
    return vals


def make_engine(p):
    """a context with the pack and NO stars"""
    return engine.Engine(p["pack"], None, None, abi.make_options(n_pops=p["n_pops"]))


# ---- 1. against the reference -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting,spec_name,n_bins,dark", [("base4", "wide", 30, True), ("base4", "window", 1, False), ("wdragged5", "wide", 30, False),
                                                           ("wdragged5", "window", 1, False), ("base9", "wide", 1, False), ("base9", "window", 30, False)])
def test_parity_with_reference(setting, spec_name, n_bins, dark):
    p, spec = problem(setting, dark), SPECS[spec_name]
    vals = reference(setting, spec_name, dark)
    n_ref = (~np.isnan(vals)).sum(axis=0)
    assert np.any((n_ref > 0) & (n_ref < len(p["rows"]))) and (spec_name != "wide" or np.any(n_ref == 0))
    exact = bc.exact_lines(spec, p["n_filt"], p["n_pops"])
    eng = make_engine(p)
    try:
        first, _ = eng.cmd_band(p["rows"][:1], br.abi_spec(spec))
        pivot = np.where(first[:, abi.BAND_N] > 0, first[:, abi.BAND_MIN], 0.0)
        ref_piv = np.where(np.isnan(vals[0]), 0.0, vals[0])
        assert np.abs(pivot - ref_piv).max() <= bc.MAG_TOL and np.array_equal(pivot[exact], ref_piv[exact])
        edges = br.safe_edges(vals, n_bins)
        mom, bins = eng.cmd_band(p["rows"], br.abi_spec(spec), pivot=pivot, edges=edges)
        want_mom, want_bins = br.accumulate(vals, pivot, edges)
        bc.check_moments(mom, want_mom, bc.pivot_deviation(vals, pivot), exact)
        bc.check_bins(bins, want_bins, vals, edges)
        # either output alone gives the same bits
        assert np.array_equal(eng.cmd_band(p["rows"], br.abi_spec(spec), pivot=pivot)[0], mom)
        assert np.array_equal(eng.cmd_band(p["rows"], br.abi_spec(spec), edges=edges, want_mom=False)[1], bins)
    finally:
        eng.close()


@pytest.mark.parametrize("setting", ["base4", "wdragged5", "base9"])
def test_quantile_brackets(setting):
    p, spec = problem(setting), SPECS["window"]
    vals = reference(setting, "window")
    eng = make_engine(p)
    try:
        res = hostlib.cmd_band(eng, p["rows"], br.abi_spec(spec), LEVELS, 1e-4, 12)
    finally:
        eng.close()
    assert bc.check_brackets(res, vals, LEVELS) > 1000
    t = hostlib.band_table(res)
    n = (~np.isnan(vals)).sum(axis=0)
    assert np.array_equal(t[:, 0], n)
    has = n > 0
    assert np.all(t[has, 3] <= t[has, 1] + 1e-9) and np.all(t[has, 1] <= t[has, 4] + 1e-9)


def test_bins_decided_on_the_values_bits():
    """An edge exactly ON a value of a copied column (the device's bits are the reference's): the value belongs to the bin the
    edge opens."""
    p, spec = problem("base4"), SPECS["wide"]
    vals = reference("base4", "wide")
    exact = bc.exact_lines(spec, p["n_filt"], p["n_pops"])
    edges = br.safe_edges(vals, 30)
    for l in np.flatnonzero(exact & ((~np.isnan(vals)).sum(axis=0) > 3))[::7]:
        v = np.sort(vals[:, l][~np.isnan(vals[:, l])])
        edges[l] = np.concatenate([[v[0] - 1.0], v[:1], v[0] + (v[-1] - v[0] + 1.0) * np.arange(1, 30) / 29.0])
    eng = make_engine(p)
    try:
        _, bins = eng.cmd_band(p["rows"], br.abi_spec(spec), edges=edges, want_mom=False)
    finally:
        eng.close()
    bc.check_bins_tied(bins, br.accumulate(vals, None, edges)[1], vals, edges, exact)


# ---- 2. ties ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ["base4", "wdragged5"])
def test_ties_to_derive_isochrone_and_predict_mags(setting):
    p, spec = problem(setting), SPECS["wide"]
    nf, n_pops, pack_d = p["n_filt"], p["n_pops"], p["pack_d"]
    P, C, n_lines = br.shape_of(spec, nf, n_pops)
    eng = make_engine(p)
    try:
        n_ms = n_strict = n_wd = 0
        for r in (0, 1, 3, 15, 17):                       # cells of 158, 2, 64-66 and 3 common EEPs
            par = p["rows"][r]
            mom, _ = eng.cmd_band(par[None, :], br.abi_spec(spec))
            got = mom[:, abi.BAND_MIN].reshape(n_pops, P, C)
            assert np.array_equal(mom[:, abi.BAND_MIN][mom[:, abi.BAND_N] > 0], mom[:, abi.BAND_MAX][mom[:, abi.BAND_N] > 0])
            off = par[abi.P_MOD] + (np.asarray(pack_d["abs_coeff"]) - 1.0) * par[abi.P_ABS]
            for k in range(n_pops):
                first, mass, mags, tip = eng.derive_isochrone(par, k)
                assert len(mass) >= 2
                e = np.arange(first, first + len(mass))
                for s, q in enumerate(spec.ratios):
                    pts = got[k, s * spec.n_eep + (e - spec.eep0)]
                    assert np.array_equal(pts[:, 0], mass)
                    if q == 0.0:
                        assert np.array_equal(pts[:, 1:1 + nf], mags + off[None, :])
                        n_ms += len(mass)
                    strict = np.flatnonzero(mass[:-1] < mass[1:])
                    pred, _ = eng.predict_mags(par, mass[strict], np.full(len(strict), q), pop=np.full(len(strict), k, np.int32))
                    assert np.array_equal(pts[strict, 1:1 + nf], pred)
                    n_strict += len(strict)
                    # outside the isochrone's EEPs: nothing
                    outside = np.setdiff1d(np.arange(spec.eep0, spec.eep0 + spec.n_eep), e)
                    assert np.all(np.isinf(got[k, s * spec.n_eep + (outside - spec.eep0)]))
                dM = (pack_d["m_wd_up"] - tip) / spec.n_wd_nodes
                m = tip + dM * np.arange(1, spec.n_wd_nodes + 1)
                for t, ty in enumerate(br.types_of(spec)):
                    pts = got[k, len(spec.ratios) * spec.n_eep + t * spec.n_wd_nodes:][:spec.n_wd_nodes]
                    there = np.isfinite(pts[:, 0])
                    assert there.any() and np.array_equal(pts[there, 0], m[there])
                    pred, stage = eng.predict_mags(par, m[there], np.zeros(int(there.sum())), wd_type=np.full(int(there.sum()), ty, np.int32),
                                                   pop=np.full(int(there.sum()), k, np.int32))
                    assert np.all(stage == abi.STAGE_WD) and np.abs(pts[there, 1:1 + nf] - pred).max() <= bc.MAG_TOL
                    n_wd += int(there.sum())
        assert n_ms > 200 and n_strict > 600 and n_wd > 200
    finally:
        eng.close()


# ---- 3. invariance, bit for bit ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_rows(setting, n_rows=300):
    p = problem(setting)
    return br.scripted_rows(p["pack_d"], p["n_pops"], (NODES[0],), n_rows)


def _both(eng, rows, spec, pivot, edges, mom=None, bins=None):
    return eng.cmd_band(rows, spec, pivot=pivot, edges=edges, mom=mom, bins=bins)


def test_splits_over_continued_calls():
    p = problem("wdragged5")
    rows = long_rows("wdragged5")
    spec = br.spec_of(0, 160, (0.0, 0.5), NODES[0], 3, ((0, 1),))
    eng = make_engine(p)
    try:
        sp = br.abi_spec(spec)
        first, _ = eng.cmd_band(rows[:1], sp)
        pivot = np.where(first[:, abi.BAND_N] > 0, first[:, abi.BAND_MIN], 0.0)
        mom0, _ = eng.cmd_band(rows, sp, pivot=pivot)
        edges = hostlib.band_first_edges(mom0, 30)
        whole = _both(eng, rows, sp, pivot, edges)
        assert whole[0][:, abi.BAND_N].max() > 256 and np.array_equal(whole[0], mom0)
        for cut in (1, 31, 32, 255, 256, 257):
            a = _both(eng, rows[:cut], sp, pivot, edges)
            b = _both(eng, rows[cut:], sp, pivot, edges, *a)
            assert np.array_equal(b[0], whole[0]) and np.array_equal(b[1], whole[1]), cut
        again = _both(eng, rows, sp, pivot, edges)           # a repeated call
        assert np.array_equal(again[0], whole[0]) and np.array_equal(again[1], whole[1])
    finally:
        eng.close()
    fresh = make_engine(p)                                   # a long-lived context against a fresh one
    try:
        got = _both(fresh, rows, br.abi_spec(spec), pivot, edges)
        assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1])
    finally:
        fresh.close()


def test_table_rule_cuts_the_chunk():
    """4096 WD nodes: a row's node table is 4096 x 15 doubles, so 64 MiB hold 136 rows and a 300-row call works in chunks of 136,
    136 and 28; three calls of 100 rows are one chunk each."""
    p = problem("base4")
    rows = long_rows("base4")
    assert (64 << 20) // (8 * 4096 * (2 * 4 + 1 + 5 + 1)) == 136
    spec = br.abi_spec(br.spec_of(0, 0, (), 4096, 1, ((1, 0),)))
    eng = make_engine(p)
    try:
        first, _ = eng.cmd_band(rows[:1], spec)
        pivot = np.where(first[:, abi.BAND_N] > 0, first[:, abi.BAND_MIN], 0.0)
        mom0, _ = eng.cmd_band(rows, spec, pivot=pivot)
        edges = hostlib.band_first_edges(mom0, 30)
        whole = _both(eng, rows, spec, pivot, edges)
        assert whole[0][:, abi.BAND_N].max() > 200
        part = None
        for r0 in range(0, 300, 100):
            part = _both(eng, rows[r0:r0 + 100], spec, pivot, edges, *(part or (None, None)))
        assert np.array_equal(part[0], whole[0]) and np.array_equal(part[1], whole[1])
    finally:
        eng.close()


def test_a_line_depends_on_its_own_point_alone():
    p, big = problem("wdragged5"), SPECS["wide"]
    rows, nf, n_pops = p["rows"], p["n_filt"], p["n_pops"]
    P, C, _ = br.shape_of(big, nf, n_pops)
    eng = make_engine(p)
    try:
        def run(spec, sel=None):
            sp = br.abi_spec(spec)
            n_lines = br.shape_of(spec, nf, n_pops)[2]
            pivot = 0.25 + 0.001 * np.arange(n_lines)
            edges = np.tile(np.linspace(-3.0, 30.0, 8), (n_lines, 1)) + 0.01 * np.arange(n_lines)[:, None]
            if sel is not None:                              # the big spec: its lines `sel` carry the small spec's pivots and edges
                pv, ed = np.zeros(sel[1]), np.tile(np.linspace(0.0, 1.0, 8), (sel[1], 1))
                pv[sel[0]], ed[sel[0]] = pivot, edges
                sp, pivot, edges = br.abi_spec(big), pv, ed
            return eng.cmd_band(rows, sp, pivot=pivot, edges=edges)

        n_big = br.shape_of(big, nf, n_pops)[2]
        # the MS/RGB point (q = 0.5, EEP 40), colour (2, 1) alone, no WD points
        small = br.spec_of(40, 1, (0.5,), 0, 0, ((2, 1),))
        Cs = br.shape_of(small, nf, n_pops)[1]
        sel = np.concatenate([br.line_index(big, nf, k, br.ms_point(big, 1, 40), 0) + np.r_[np.arange(1 + nf), 1 + nf + 1] for k in range(n_pops)])
        a, b = run(small), run(small, (sel, n_big))
        assert a[0].shape == (n_pops * Cs, 5) and a[0][:, abi.BAND_N].max() > 10
        assert np.array_equal(a[0], b[0][sel]) and np.array_equal(a[1], b[1][sel])
        # the DB sequence alone, no colours: the big spec has it as its second type
        small = br.spec_of(0, 0, (), NODES[0], 2, ())
        cols = np.arange(1 + nf)
        sel = np.concatenate([br.line_index(big, nf, k, br.wd_point(big, 1, j), 0) + cols for k in range(n_pops) for j in range(1, NODES[0] + 1)])
        a, b = run(small), run(small, (sel, n_big))
        assert a[0][:, abi.BAND_N].max() > 10
        assert np.array_equal(a[0], b[0][sel]) and np.array_equal(a[1], b[1][sel])
    finally:
        eng.close()


def test_sampler_blocks_are_untouched():
    from base_amd import mcmc
    prob = rch.problem("base4")
    p = problem("base4")
    pack, stars, priors, options = rch.device_args(prob, 2, 2)
    free = np.array(mcmc.DEFAULT_FREE)
    chol = np.diag([mcmc.DEFAULT_STEP[k] for k in free]) * 0.3
    start = synth.walker_params(prob["truth"], 4, seed=2, scale=0.3)
    spec = br.abi_spec(SPECS["wide"])

    def run(interleave):
        eng = engine.Engine(pack, stars, priors, options)
        try:
            lp0 = eng.logpost(start)
            h = eng.mcmc_submit(start, lp0, np.arange(4), free, chol, 11, 0, 6, asynchronous=True)
            if interleave:
                with pytest.raises(engine.B9Error) as e:       # B9_ERR_STATE: a block is outstanding
                    eng.cmd_band(p["rows"], spec)
                assert e.value.code == abi.B9_ERR_STATE and "outstanding" in str(e.value)
            first = [np.array(x) for x in eng.mcmc_collect(h)[:4]]
            if interleave:
                mom, _ = eng.cmd_band(p["rows"], spec)
                assert mom[:, abi.BAND_N].max() >= 30
            h = eng.mcmc_submit(start, lp0, np.arange(4), free, chol, 11, 6, 6, cont=True, asynchronous=True)
            second = [np.array(x) for x in eng.mcmc_collect(h)[:4]]
        finally:
            eng.close()
        return first + second

    for a, b in zip(run(False), run(True)):
        assert np.array_equal(a, b)


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    p = problem("base4")
    rows = np.ascontiguousarray(p["rows"])
    nf = p["n_filt"]
    eng = make_engine(p)
    try:
        def call(n_rows=4, spec=None, mom=True, bins=True, params=True, have_spec=True, have_edges=True, n_bins=4, edges=None, ctx=True, **kw):
            args = dict(eep0=10, n_eep=5, ratios=(0.0, 1.0), n_wd_nodes=3, wd_types=1, colours=((0, 1),))
            args.update(kw)
            sp = abi.make_band_spec(**args) if spec is None else spec
            n_lines = max(1, abi.band_shape(sp.struct, nf, 1)[2]) if 0 <= sp.struct.n_ratio <= 4 and sp.struct.n_eep >= 0 and sp.struct.n_wd_nodes >= 0 else 64
            e = np.tile(np.linspace(0.0, 30.0, max(n_bins, 1) + 1), (n_lines, 1)) if edges is None else np.ascontiguousarray(edges, dtype=np.float64)
            m, b = np.full((n_lines, 5), 7.25), np.full((n_lines, max(n_bins, 1) + 3), 7.25)
            code = eng.lib.b9_cmd_band(eng._ctx if ctx else None, rows.ctypes.data_as(_dp) if params else None, n_rows, C.byref(sp.struct) if have_spec else None,
                                       0, None, m.ctypes.data_as(_dp) if mom else None, e.ctypes.data_as(_dp) if have_edges else None, n_bins,
                                       b.ctypes.data_as(_dp) if bins else None)
            assert code == abi.B9_OK or (np.all(m == 7.25) and np.all(b == 7.25))
            return code

        INV = abi.B9_ERR_INVALID
        assert call() == abi.B9_OK and call(mom=False) == abi.B9_OK and call(bins=False) == abi.B9_OK
        assert call(bins=False, have_edges=False, n_bins=0) == abi.B9_OK                  # edges and n_bins matter only with bins
        assert call(n_rows=0) == INV and call(n_rows=-1) == INV
        assert call(params=False) == INV and call(have_spec=False) == INV and call(ctx=False) == INV
        assert call(mom=False, bins=False) == INV
        assert call(n_eep=0, ratios=(), n_wd_nodes=0) == INV                              # no lines
        assert "no lines" in eng.lib.b9_last_error(eng._ctx).decode()
        assert call(n_eep=0, n_wd_nodes=0) == INV                                         # ratios without EEPs and no WD nodes: no lines either
        assert call(n_eep=-1) == INV
        bad = abi.make_band_spec(10, 5, (0.0, 1.0), 3, 1, ((0, 1),))
        bad.struct.n_ratio = 5
        assert call(spec=bad) == INV
        bad.struct.n_ratio = -1
        assert call(spec=bad) == INV
        assert call(ratios=(0.0, 1.5)) == INV and call(ratios=(-0.1,)) == INV and call(ratios=(np.nan,)) == INV and call(ratios=(np.inf,)) == INV
        assert call(ratios=()) == INV                                                    # n_eep > 0 with n_ratio = 0
        assert call(n_wd_nodes=-1) == INV
        assert call(wd_types=0) == INV and call(wd_types=4) == INV and call(wd_types=-1) == INV
        assert call(n_wd_nodes=0, wd_types=0) == abi.B9_OK                                # the types matter only with nodes
        bad = abi.make_band_spec(10, 5, (0.0, 1.0), 3, 1, ((0, 1),))
        bad.struct.n_colour = 9
        assert call(spec=bad) == INV
        bad.struct.n_colour = -1
        assert call(spec=bad) == INV
        assert call(colours=((0, nf),)) == INV and call(colours=((-1, 0),)) == INV and call(colours=((2, 2),)) == INV
        assert call(colours=[(f, f + 1) for f in range(3)] * 2 + [(0, 2), (3, 1)]) == abi.B9_OK      # eight colours
        assert call(have_edges=False) == INV                                             # bins without edges
        assert call(n_bins=0) == INV and call(n_bins=31) == INV and call(n_bins=30) == abi.B9_OK
        n_lines = abi.band_shape(abi.make_band_spec(10, 5, (0.0, 1.0), 3, 1, ((0, 1),)).struct, nf, 1)[2]
        for v, where in ((np.nan, 2), (np.inf, 4), (None, 3)):
            e = np.tile(np.linspace(0.0, 30.0, 5), (n_lines, 1))
            e[n_lines - 1, where] = e[n_lines - 1, where - 1] if v is None else v
            assert call(edges=e) == INV
        assert "ascending" in eng.lib.b9_last_error(eng._ctx).decode()
        assert call(edges=np.tile(np.linspace(30.0, 0.0, 5), (n_lines, 1))) == INV
    finally:
        eng.close()
    # no pack: B9_ERR_STATE
    bare = engine.Engine()
    try:
        with pytest.raises(engine.B9Error) as e:
            bare.n_filt = nf
            bare.cmd_band(rows, abi.make_band_spec(10, 5, (0.0,), 0, 0, ()))
        assert e.value.code == abi.B9_ERR_STATE
    finally:
        bare.close()


# ---- 5. the program ---------------------------------------------------------------------------------------------------------------
def test_cli_cmd_band(tmp_path):
    """simCluster -> scatterCluster -> singlePopMcmc (short: 4 walkers x 100 main-run rows, two chunks of the call) -> cmdBand with two ratios, 32 WD nodes of both types and a colour: the file parses, holds the
    spec's lines in order, every line is final, equals hostlib.cmd_band's table of the same rows to the bit, and the median of the
    single-star turn-off EEP lies inside [min, max] of the same line."""
    from base_amd import build, host_build
    build.build_hip()
    host_build.build_host()
    pack_d = synth.make_pack("parsec", 8, n_feh=4, n_age=8, n_eep=90)
    truth = synth.default_params(pack_d)
    truth[abi.P_IFMR_INTERCEPT], truth[abi.P_IFMR_SLOPE], truth[abi.P_IFMR_QUAD] = 0.77, 0.08, 0.0   # the session's defaults
    root = synth.write_models_dir(pack_d, str(tmp_path / "models"))
    base = str(tmp_path / "run")
    y_true = synth.write_yaml(str(tmp_path / "truth.yaml"), base + ".sim.scatter", root, base, truth, seed=17)
    r = _cli("simCluster", "--config", y_true, "--nStars", "120", "--percentBinary", "30", "--minMass", "0.4")
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
    filters = list(pack_d["filters"])
    colour = f"{filters[1]}-{filters[2]}"
    r = _cli("cmdBand", "--config", y, "--ratios", "0,1", "--wdNodes", "32", "--wdTypes", "both", "--colours", colour)
    assert r.returncode == 0, r.stderr
    assert "0 lines unfinished" in r.stderr
    names, cols, table = hostlib.read_cmd_band(fit + ".cmdBand")
    m = len(hostlib.STAR_INTERVALS_LEVELS)
    assert cols[:5] == ["N", "mean", "sd", "min", "max"] and cols[-2:] == ["passes", "flags"] and len(cols) == 5 + 3 * m + 2
    eep_lo = int(np.min(pack_d["iso_first_eep"]))
    eep_hi = int(np.max(np.asarray(pack_d["iso_first_eep"]) + np.asarray(pack_d["iso_n_eep"])))
    nf = len(filters)
    C_ = 1 + nf + 1
    assert len(names) == (2 * (eep_hi - eep_lo) + 2 * 32) * C_
    assert names[0] == f"p0.q0.eep{eep_lo}.mass" and names[1] == f"p0.q0.eep{eep_lo}.{filters[0]}" and names[C_ - 1] == f"p0.q0.eep{eep_lo}.{colour}"
    assert names[-1] == f"p0.db.n32.{colour}"
    assert np.all((table[:, -1].astype(int) & hostlib.SIV_OPEN) == 0)                     # every line is final
    rows = hostlib.read_res_rows(fit + ".res", start, 3)
    assert len(rows) == 100 * 4
    spec = abi.make_band_spec(eep_lo, eep_hi - eep_lo, (0.0, 1.0), 32, 3, ((1, 2),))
    eng = engine.Engine(abi.make_pack(pack_d), None, None, abi.make_options(n_pops=1))
    try:
        res = hostlib.cmd_band(eng, rows, spec)
    finally:
        eng.close()
    assert np.array_equal(table, hostlib.band_table(res), equal_nan=True)              # 17 digits: the program's loop is the library's
    # the turn-off: the single-star locus' bluest point in (filter 1 - filter 2) among the EEPs every row has
    n = table[:, 0].reshape(-1, C_)
    med = table[:, 5 + 3 * list(hostlib.STAR_INTERVALS_LEVELS).index(0.5)].reshape(-1, C_)
    lo, hi = table[:, 3].reshape(-1, C_), table[:, 4].reshape(-1, C_)
    single = np.arange(eep_hi - eep_lo)
    full = single[n[single, C_ - 1] == len(rows)]
    assert len(full) > 20
    to = full[np.argmin(med[full, C_ - 1])]
    for c in range(C_):
        assert lo[to, c] <= med[to, c] <= hi[to, c], (to, c)
    print(f"turn-off EEP {eep_lo + to}: colour median {med[to, C_ - 1]:.5f} in [{lo[to, C_ - 1]:.5f}, {hi[to, C_ - 1]:.5f}], mass {med[to, 0]:.5f}")
