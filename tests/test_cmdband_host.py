"""CPU tests of cmdBand's reference (tests/band_ref.py), comparators (tests/band_check.py) and host functions (b9h_band_first_edges,
b9h_band_table, the writer, the settings parser, hostlib.cmd_band's loop on the reference).  No GPU."""
import functools
import math

import numpy as np
import pytest

import band_check as bc
import band_ref as br
import ragged_walk as rw
import wd_check
from base_amd import abi, hostlib, synth

N_FILT = 4
LEVELS = (0.0313, 0.1687, 0.5171, 0.8329, 0.9771)           # a N is no integer for any N below 10000


@functools.lru_cache(maxsize=None)
def problem(dark=True):
    pack_d = rw.ladder_pack(N_FILT, 1, 0, "base")
    if dark:
        pack_d = br.dark_pack(pack_d)
    rows = br.scripted_rows(pack_d, 1, (63,))
    spec = br.spec_of(8, 40, (0.0, 0.5, 1.0), 63, 3, ((0, 1), (2, 1)))
    facts = {}
    vals = br.values(pack_d, rows, 1, spec, facts=facts)
    vals.setflags(write=False)
    return dict(pack_d=pack_d, rows=rows, spec=spec, vals=vals, facts=facts)


def pivots(vals):
    first = vals[0]
    return np.where(np.isnan(first), 0.0, first)


# ---- the reference against an independent statement -----------------------------------------------------------------------------
def test_reference_against_brute_force_on_three_rows():
    """Three rows (a long cell, a 3-point cell, outside the grid), every line: the values restated from synth's own numpy isochrone
    and wd_check's WD chain, the moments and bins by scalar loops."""
    p = problem(False)
    pack_d, spec = p["pack_d"], p["spec"]
    rows = p["rows"][[0, 15, 8]]
    vals = br.values(pack_d, rows, 1, spec)
    P, C, n_lines = br.shape_of(spec, N_FILT, 1)
    assert abi.band_shape(br.abi_spec(spec).struct, N_FILT, 1) == (P, C, n_lines)      # the binding counts the lines as the reference does
    want = np.full((3, n_lines), np.nan)
    for r, par in enumerate(rows):
        iso = synth.derive_isochrone(pack_d, par[abi.P_LOGAGE], par[abi.P_FEH], par[abi.P_Y])
        if iso is None:
            continue
        first, mass, mags = iso
        off = par[abi.P_MOD] + (pack_d["abs_coeff"] - 1.0) * par[abi.P_ABS]
        for s, q in enumerate(spec.ratios):
            for e in range(spec.eep0, spec.eep0 + spec.n_eep):
                if not first <= e < first + len(mass):
                    continue
                flux = 10.0 ** (-0.4 * mags[e - first])
                m2 = q * mass[e - first]
                if q > 0 and m2 >= mass[0]:
                    flux = flux + 10.0 ** (-0.4 * np.array([np.interp(m2, mass, mags[:, f]) for f in range(N_FILT)]))
                app = -2.5 * np.log10(flux) + off
                o = ((s * spec.n_eep + e - spec.eep0) * C)
                want[r, o] = mass[e - first]
                want[r, o + 1:o + 1 + N_FILT] = app
                want[r, o + 1 + N_FILT:o + C] = [app[a] - app[b] for a, b in spec.colours]
        tip = mass[-1]
        dM = (pack_d["m_wd_up"] - tip) / spec.n_wd_nodes
        for t in range(2):
            for j in range(1, spec.n_wd_nodes + 1):
                m = tip + dM * j
                wdm, prec, cool, lteff, logg = (x[0] for x in wd_check.wd_chain(pack_d, par, [m]))
                if not (m <= pack_d["m_wd_up"] and prec < par[abi.P_LOGAGE]):
                    continue
                app = wd_check.apparent(pack_d, par, wd_check.atmosphere_mags(pack_d, lteff, logg, t))[0]
                o = (len(spec.ratios) * spec.n_eep + t * spec.n_wd_nodes + j - 1) * C
                want[r, o] = m
                want[r, o + 1:o + 1 + N_FILT] = app
                want[r, o + 1 + N_FILT:o + C] = [app[a] - app[b] for a, b in spec.colours]
    assert np.array_equal(np.isnan(vals), np.isnan(want))
    assert np.isnan(vals[2]).all() and not np.isnan(vals[0]).all()
    ok = ~np.isnan(want)
    assert np.abs(vals[ok] - want[ok]).max() < 1e-11
    # the accumulation, by scalar loops
    piv = pivots(vals)
    edges = br.safe_edges(vals, 5)
    mom, bins = br.accumulate(vals, piv, edges)
    for l in range(0, n_lines, 7):
        n = sm = sq = 0.0
        mn, mx = math.inf, -math.inf
        words = [0.0] * 8
        for r in range(3):
            v = float(vals[r, l])
            if v != v:
                continue
            d = v - float(piv[l])
            n += 1.0; sm += d; sq += d * d; mn = min(mn, v); mx = max(mx, v)
            w = 0
            while w <= 5 and float(edges[l, w]) <= v:
                w += 1
            words[w] += 1.0; words[7] += 1.0
        assert list(mom[l]) == [n, sm, sq, mn, mx], l
        assert list(bins[l]) == words, l


def test_reference_is_not_vacuous():
    p = problem()
    vals, spec = p["vals"], p["spec"]
    n = (~np.isnan(vals)).sum(axis=0)
    n_rows = vals.shape[0]
    assert abi.band_shape(br.abi_spec(spec).struct, N_FILT, 1)[2] == len(n)
    assert np.any((n > 0) & (n < n_rows)) and np.any(n == 0) and np.any(n >= 30)
    assert p["facts"]["uncooled"] > 0 and p["facts"]["secondary_below_first"] > 0
    # some WD line loses rows to uncooled nodes: it has fewer rows than the rows inside the grid
    P, C, _ = br.shape_of(spec, N_FILT, 1)
    inside = n[br.line_index(spec, N_FILT, 0, br.ms_point(spec, 0, 9), 0)]          # EEP 9 is common to every cell of two or more points
    wd_n = n.reshape(P, C)[len(spec.ratios) * spec.n_eep:, 0]
    assert np.any((wd_n > 0) & (wd_n < inside))
    # the dark filter: the single star's column is absent where its mass column is not, the binary's is not (the secondary shines)
    o = br.line_index(spec, N_FILT, 0, br.ms_point(spec, 0, 30), 0)
    assert n[o] > 0 and n[o + 1 + 1] == 0 and n[o + 1 + 0] == n[o]
    assert n[o + 1 + N_FILT] == 0 and n[o + 1 + N_FILT + 1] == 0                   # both colours take filter 1
    o5 = br.line_index(spec, N_FILT, 0, br.ms_point(spec, 1, 30), 0)
    assert n[o5 + 1 + 1] == n[o5] > 0


# ---- every stand-in is rejected ---------------------------------------------------------------------------------------------------
def _outputs(p, mutate, edges, piv):
    vals = br.values(p["pack_d"], p["rows"], 1, p["spec"], mutate=mutate) if mutate in br.MUTATIONS[:4] else p["vals"]
    return br.accumulate(vals, piv, edges, mutate=mutate)


def test_comparators_accept_the_reference_and_reject_every_stand_in():
    p = problem()
    vals, spec = p["vals"], p["spec"]
    piv = pivots(vals)
    edges = br.safe_edges(vals, 30)
    dev = bc.pivot_deviation(vals, piv)
    exact = bc.exact_lines(spec, N_FILT, 1)
    mom, bins = br.accumulate(vals, piv, edges)
    bc.check_moments(mom, mom, dev, exact)
    bc.check_bins(bins, bins, vals, edges)
    rejected_by = {"moments": set(), "bins": set(), "brackets": set()}
    for mut in br.MUTATIONS:
        m2, b2 = _outputs(p, mut, edges, piv)
        if bc.rejects(bc.check_moments, m2, mom, dev, exact):
            rejected_by["moments"].add(mut)
        if mut != "bin_closed_right" and bc.rejects(bc.check_bins, b2, bins, vals, edges):
            rejected_by["bins"].add(mut)
    # a bin closed on the right shows only where a value sits ON an edge: the copied columns allow that (the device's bits are
    # the reference's), through the comparator that admits exact ties on exactly those lines
    tied = edges.copy()
    lines = np.flatnonzero(exact & ((~np.isnan(vals)).sum(axis=0) > 3))[:50]
    for l in lines:
        v = np.sort(vals[:, l][~np.isnan(vals[:, l])])
        tied[l] = np.concatenate([[v[0] - 1.0], v[:1], v[0] + (v[-1] - v[0] + 1.0) * np.arange(1, 30) / 29.0])[:31]
        assert np.all(np.diff(tied[l]) > 0)
    _, bt = br.accumulate(vals, piv, tied)
    bc.check_bins_tied(bt, bt, vals, tied, exact)
    assert bc.rejects(bc.check_bins_tied, br.accumulate(vals, piv, tied, mutate="bin_closed_right")[1], bt, vals, tied, exact)
    rejected_by["bins"].add("bin_closed_right")
    with pytest.raises(AssertionError):                    # ... and the plain comparator refuses such edges outright
        bc.assert_edges_clear(vals, tied)
    # the brackets: the loop on a faulty engine
    good = hostlib.cmd_band(br.RefEngine(p["pack_d"], 1), p["rows"], spec, LEVELS, 1e-4, 12)
    assert bc.check_brackets(good, vals, LEVELS) > 1000
    for mut in br.MUTATIONS:
        if mut == "pivot_ignored":
            continue                                       # the brackets do not depend on the pivots
        res = hostlib.cmd_band(br.RefEngine(p["pack_d"], 1, mut), p["rows"], spec, LEVELS, 1e-4, 12)
        if bc.rejects(bc.check_brackets, res, vals, LEVELS):
            rejected_by["brackets"].add(mut)
    # the stand-ins that keep every value and change only how the sums are formed: inside every tolerance, so that nothing but
    # the bit-for-bit comparison of the copied columns' SUM and SUMSQ rejects them
    for mut in br.ORDER_MUTATIONS:
        m2, b2 = br.accumulate(vals, piv, edges, mutate=mut)
        assert np.array_equal(m2[:, [br.N, br.MIN, br.MAX]], mom[:, [br.N, br.MIN, br.MAX]]) and np.array_equal(b2, bins)
        bc.check_moments(m2, mom, dev, None)                                   # the tolerances alone accept it
        with pytest.raises(AssertionError, match="SUMSQ of a copied column" if mut == "fused_square" else "SUM of a copied column"):
            bc.check_moments(m2, mom, dev, exact)
        differ = (m2[:, br.SUMSQ] != mom[:, br.SUMSQ]) if mut == "fused_square" else (m2[:, br.SUM] != mom[:, br.SUM])
        assert (differ & exact).sum() > 50, mut
    assert rejected_by["moments"] >= {"last_eep_dropped", "uncooled_counted", "noflux_enters", "absolute_colour", "pivot_ignored"}, rejected_by
    assert rejected_by["bins"] >= {"last_eep_dropped", "uncooled_counted", "noflux_enters", "absolute_colour", "bin_closed_right"}, rejected_by
    assert rejected_by["brackets"] >= {"last_eep_dropped", "uncooled_counted", "noflux_enters", "absolute_colour"}, rejected_by


# ---- the host functions -----------------------------------------------------------------------------------------------------------
def test_band_first_edges():
    p = problem()
    mom, _ = br.accumulate(p["vals"], pivots(p["vals"]))
    for B in (1, 7, 30):
        e = hostlib.band_first_edges(mom, B)
        assert e.shape == (len(mom), B + 1) and np.all(np.diff(e, axis=1) > 0) and np.isfinite(e).all()
        has = mom[:, br.N] > 0
        assert np.all(e[has, 0] < mom[has, br.MIN]) and np.all(e[has, -1] > mom[has, br.MAX])
        assert np.array_equal(e[~has], np.tile(np.arange(B + 1) / B, ((~has).sum(), 1)))
        lo, hi = hostlib.band_first_ranges(mom)                                # the loop's first ranges: their even cut is these edges
        assert np.array_equal(e, lo[:, None] + (hi - lo)[:, None] * (np.arange(B + 1) / float(B))[None, :])
    one = np.array([[1.0, 0.0, 0.0, 12.5, 12.5], [0.0, 0.0, 0.0, np.inf, -np.inf]])
    e = hostlib.band_first_edges(one, 30)
    assert e[0, 0] < 12.5 < e[0, -1] and np.all(np.diff(e[0]) > 0) and list(e[1, [0, -1]]) == [0.0, 1.0]
    with pytest.raises(hostlib.HostError):
        hostlib.band_first_edges(one, 31)


def test_band_table_writer_and_loop(tmp_path):
    p = problem()
    vals, spec = p["vals"], p["spec"]
    res = hostlib.cmd_band(br.RefEngine(p["pack_d"], 1), p["rows"], spec, LEVELS, 1e-4, 12)
    assert np.array_equal(res["pivot"], pivots(vals))
    t = hostlib.band_table(res)
    m = len(LEVELS)
    assert t.shape == (vals.shape[1], 5 + 3 * m + 2)
    n = (~np.isnan(vals)).sum(axis=0)
    assert np.array_equal(t[:, 0], n)
    has = n > 0
    with np.errstate(invalid="ignore"):
        mean, sd = np.nanmean(vals[:, has], axis=0), np.nanstd(vals[:, has], axis=0)
    assert np.allclose(t[has, 1], mean, rtol=0, atol=1e-9) and np.allclose(t[has, 2], sd, rtol=0, atol=1e-6)
    assert np.array_equal(t[has, 3], np.nanmin(vals[:, has], axis=0)) and np.array_equal(t[has, 4], np.nanmax(vals[:, has], axis=0))
    assert np.isnan(t[~has, 1]).all() and np.isnan(t[~has, 2]).all() and np.all(t[~has, 3] == np.inf) and np.all(t[~has, 4] == -np.inf)
    assert np.array_equal(t[:, 5::3][:, :m], res["value"], equal_nan=True) and np.array_equal(t[:, -2], res["passes"]) and np.array_equal(t[:, -1], res["flags"])
    assert np.all((res["flags"][has] & hostlib.SIV_OPEN) == 0)
    names = [f"p0.l{i}" for i in range(len(t))]
    path = str(tmp_path / "x.cmdBand")
    hostlib.write_cmd_band(path, names, LEVELS, t)
    got_names, cols, back = hostlib.read_cmd_band(path)
    assert got_names == names and cols[:5] == ["N", "mean", "sd", "min", "max"] and cols[-2:] == ["passes", "flags"]
    assert cols[5:8] == ["q0.0313", "q0.0313_lo", "q0.0313_hi"]
    assert np.array_equal(back, t, equal_nan=True)


def test_settings(tmp_path):
    d = hostlib.cmd_band_settings([])
    assert d == dict(ratios=(0.0, 1.0), wdNodes=256, wdTypes=1, colours=(), levels=(0.025, 0.16, 0.5, 0.84, 0.975), tol=1e-4, maxPasses=12, nPops=1)
    d = hostlib.cmd_band_settings(["--ratios", "0,0.5,1", "--wdNodes", "64", "--wdTypes", "both", "--colours", "B-V,V-I", "--levels", "0.1,0.9",
                                   "--tol", "1e-6", "--maxPasses", "5", "--nPops", "2"])
    assert d == dict(ratios=(0.0, 0.5, 1.0), wdNodes=64, wdTypes=3, colours=("B-V", "V-I"), levels=(0.1, 0.9), tol=1e-6, maxPasses=5, nPops=2)
    cfg = tmp_path / "c.yaml"
    cfg.write_text("cmdBand:\n    ratios: [0, 0.7]\n    wdNodes: 0\n    wdTypes: db\n")
    d = hostlib.cmd_band_settings(["--config", str(cfg)])
    assert d["ratios"] == (0.0, 0.7) and d["wdNodes"] == 0 and d["wdTypes"] == 2
    for bad in (["--ratios", "1.5"], ["--ratios", "0,0.1,0.2,0.3,0.4"], ["--wdTypes", "dc"], ["--colours", "BV"], ["--wdNodes", "-1"],
                ["--maxPasses", "0"], ["--tol", "-1"], ["--nPops", "3"], ["--levels", "0.5,0.4"], ["--ratios", "", "--wdNodes", "0"]):
        with pytest.raises(hostlib.HostError):
            hostlib.cmd_band_settings(bad)
