"""numpy reference of b9_cmd_band (include/base9_hip.h): the value of every (row, line), the moments and bins accumulated by the
call's own plain sequence, and every line's exact order statistics.  Pure numpy and the CPU oracle: nothing here needs a GPU.

The MS/RGB points are the oracle's isochrone (oracle.derive_isochrone: the device's, bit for bit), the secondaries synth's
single-star rule on that isochrone (synth._single_mags, forward_mags' MS/RGB piece) combined as forward_mags combines fluxes,
the WD nodes synth.forward_mags at the node's mass with the COOLED rule of tests/wdmoments_ref.py (m <= M_wd_up, prec < logAge,
the pack has WD tables).  `mutate` names one faulty stand-in (MUTATIONS) that tests/test_cmdband_host.py shows the comparators
reject."""
import collections
import math

import numpy as np

import oracle
import wd_check
import wdmoments_ref as wr
from base_amd import abi, synth

N, SUM, SUMSQ, MIN, MAX, NMOM = range(6)
MUTATIONS = ("last_eep_dropped", "uncooled_counted", "noflux_enters", "absolute_colour", "bin_closed_right", "pivot_ignored")
#: stand-ins that keep every value and differ only in HOW the sums are formed: the rows taken in descending order, the square
#: contracted into the sum (one rounding, fma(d, d, SUMSQ)).  Only a bit-for-bit comparison of SUM / SUMSQ tells them apart.
ORDER_MUTATIONS = ("rows_reversed", "fused_square")

Spec = collections.namedtuple("Spec", "eep0 n_eep ratios n_wd_nodes wd_types colours")


def spec_of(eep0=0, n_eep=0, ratios=(), n_wd_nodes=0, wd_types=0, colours=()):
    return Spec(int(eep0), int(n_eep), tuple(float(q) for q in ratios), int(n_wd_nodes), int(wd_types), tuple((int(a), int(b)) for a, b in colours))


def abi_spec(spec):
    return abi.make_band_spec(spec.eep0, spec.n_eep, spec.ratios, spec.n_wd_nodes, spec.wd_types, spec.colours)


def types_of(spec):
    return [t for t in range(2) if spec.n_wd_nodes > 0 and spec.wd_types >> t & 1]


def shape_of(spec, n_filt, n_pops):
    """(P, C, n_lines)"""
    P = len(spec.ratios) * spec.n_eep + len(types_of(spec)) * spec.n_wd_nodes
    C = 1 + n_filt + len(spec.colours)
    return P, C, n_pops * P * C


def line_index(spec, n_filt, k, p, c):
    P, C, _ = shape_of(spec, n_filt, 1)
    return (k * P + p) * C + c


def ms_point(spec, s, e):
    return s * spec.n_eep + (e - spec.eep0)


def wd_point(spec, t, j):
    return len(spec.ratios) * spec.n_eep + t * spec.n_wd_nodes + (j - 1)


def offsets(pack_d, par):
    """mod + (A_f / A_V - 1) A_V, in the device's grouping"""
    return par[abi.P_MOD] + (np.asarray(pack_d["abs_coeff"], dtype=np.float64) - 1.0) * par[abi.P_ABS]


def _columns(app, enters, colours, absolute=None):
    """one point's columns after the mass: the magnitudes that enter, then the colours (NaN: absent)"""
    mags = np.where(enters, app, np.nan)
    src = mags if absolute is None else np.where(enters, absolute, np.nan)
    return np.concatenate([mags, [src[a] - src[b] for a, b in colours]])


def row_values(pack_d, pinned, olib, par, n_pops, spec, mutate=None, facts=None):
    """values [n_lines] of one parameter row, NaN where the line takes nothing from it.  facts (a dict, optional) counts what the
    row exercised: secondaries below the isochrone's first mass, WD nodes that exist but have not cooled."""
    par = np.asarray(par, dtype=np.float64)
    nf = pack_d["n_filt"]
    P, C, n_lines = shape_of(spec, nf, n_pops)
    out = np.full(n_lines, np.nan)
    off = offsets(pack_d, par)
    for k in range(n_pops):
        first, mass, mags, tip = oracle.derive_isochrone(olib, pinned, par, k)
        n = len(mass)
        if n == 0:
            continue
        par_k = par.copy()
        if k:
            par_k[abi.P_Y] = par[abi.P_Y2]
        n_used = n - 1 if mutate == "last_eep_dropped" else n
        for s, q in enumerate(spec.ratios):
            for e in range(max(spec.eep0, first), min(spec.eep0 + spec.n_eep, first + n_used)):
                i = e - first
                p1 = mags[i].copy()
                dark = p1 == abi.MAG_NOFLUX
                if q > 0.0:
                    p2 = synth._single_mags(pack_d, par_k, (first, mass, mags), np.array([q * mass[i]]), np.zeros(1, np.int32))[0]
                    if facts is not None and q * mass[i] < mass[0]:
                        facts["secondary_below_first"] = facts.get("secondary_below_first", 0) + 1
                    dark = dark & (p2 == abi.MAG_NOFLUX)
                    p1 = -2.5 * np.log10(10.0 ** (-0.4 * p1) + 10.0 ** (-0.4 * p2))
                app = np.where(dark, abi.MAG_NOFLUX, p1 + off)
                enters = np.isfinite(app) & (app != abi.MAG_NOFLUX)
                if mutate == "noflux_enters":
                    enters = np.isfinite(app)
                o = line_index(spec, nf, k, ms_point(spec, s, e), 0)
                out[o] = mass[i]
                out[o + 1:o + C] = _columns(app, enters, spec.colours, p1 if mutate == "absolute_colour" else None)
        if spec.n_wd_nodes > 0 and types_of(spec):
            nn = spec.n_wd_nodes
            dM = (pack_d["m_wd_up"] - tip) / nn
            if not dM > 0.0:
                continue
            m = tip + dM * np.arange(1, nn + 1, dtype=np.float64)
            is_wd = (m > tip) & (m <= pack_d["m_wd_up"])
            prec = wd_check.wd_chain(pack_d, par, m, pop=k)[1]
            cooled = is_wd & (prec < par[abi.P_LOGAGE]) & wr.has_wd_tables(pack_d)
            if facts is not None:
                facts["uncooled"] = facts.get("uncooled", 0) + int((is_wd & ~cooled).sum())
            take = is_wd if mutate == "uncooled_counted" else cooled
            for t, ty in enumerate(types_of(spec)):
                if not take.any():
                    continue
                app = np.full((nn, nf), np.nan)
                app[take] = synth.forward_mags(pack_d, par, m[take], np.zeros(int(take.sum())), np.full(int(take.sum()), ty, np.int32), pop=k)
                for j in np.flatnonzero(take):
                    enters = np.isfinite(app[j]) & (app[j] != abi.MAG_NOFLUX)
                    o = line_index(spec, nf, k, wd_point(spec, t, j + 1), 0)
                    out[o] = m[j]
                    out[o + 1:o + C] = _columns(app[j], enters, spec.colours, app[j] - off if mutate == "absolute_colour" else None)
    return out


def values(pack_d, rows, n_pops, spec, mutate=None, facts=None):
    """[n_rows, n_lines]"""
    pinned = abi.make_pack(pack_d)
    olib = oracle.load()
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, abi.B9_NPARAM)
    return np.stack([row_values(pack_d, pinned, olib, par, n_pops, spec, mutate, facts) for par in rows])


def start_mom(n_lines):
    mom = np.zeros((n_lines, NMOM))
    mom[:, MIN], mom[:, MAX] = np.inf, -np.inf
    return mom


def bin_word(edges, v, closed_right=False):
    """the word a value adds 1.0 to: 0 below, 1 + b for e_b <= v < e_(b+1), B + 1 at or above; edges [.., B + 1], v [..]"""
    return ((edges < v[..., None]) if closed_right else (edges <= v[..., None])).sum(axis=-1)


def _fma(a, b, c):
    """fma(a, b, c) of arrays, exactly rounded (rational arithmetic: only the fused_square stand-in pays for it)"""
    from fractions import Fraction
    return np.array([float(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)], dtype=np.float64)


def accumulate(vals, pivot=None, edges=None, mom=None, bins=None, mutate=None):
    """(mom [n_lines, 5], bins [n_lines, B + 3] or None): the call's plain sequence, one IEEE operation per row and column in
    ascending row order, continued from mom / bins when given."""
    n_rows, n_lines = vals.shape
    piv = np.zeros(n_lines) if pivot is None or mutate == "pivot_ignored" else np.asarray(pivot, dtype=np.float64)
    mom = start_mom(n_lines) if mom is None else np.array(mom, dtype=np.float64)
    if edges is not None:
        edges = np.asarray(edges, dtype=np.float64).reshape(n_lines, -1)
        B = edges.shape[1] - 1
        bins = np.zeros((n_lines, B + 3)) if bins is None else np.array(bins, dtype=np.float64)
    for r in (range(n_rows - 1, -1, -1) if mutate == "rows_reversed" else range(n_rows)):
        v = vals[r]
        sel = np.flatnonzero(~np.isnan(v))
        d = v[sel] - piv[sel]
        mom[sel, N] += 1.0
        mom[sel, SUM] += d
        if mutate == "fused_square":
            mom[sel, SUMSQ] = _fma(d, d, mom[sel, SUMSQ])
        else:
            mom[sel, SUMSQ] += d * d
        mom[sel, MIN] = np.fmin(mom[sel, MIN], v[sel])
        mom[sel, MAX] = np.fmax(mom[sel, MAX], v[sel])
        if edges is not None:
            w = bin_word(edges[sel], v[sel], mutate == "bin_closed_right")
            bins[sel, w] += 1.0
            bins[sel, B + 2] += 1.0
    return mom, (bins if edges is not None else None)


# ---- the scripted rows of the tests: 40 hops between the ladder pack's cells (tests/ragged_walk.py) and out of the grid ----------
OUT, INVALID_CELL = "O", 10
TOKENS = [3, 9, 3, 2, 1, 2, INVALID_CELL, 4, OUT, 5, 6, 5, 7, 0, 3, 8, INVALID_CELL, 9, OUT, 9, 4, 1, 6, 3, 7, 0, 8, 6, 2, 5, 1, 3, 9, 4, OUT, 5, 2,
          8, 0, 3]
SEAM_TOL = 1e-6           # no reference node has |prec - logAge| within this: its COOLED status is not a matter of rounding


def wd_screen(pack_d, par, n_pops, node_counts):
    """Is every WD node of the row, at every node count and population, clear of the prec = logAge seam and outside the band of
    masses whose precursor age has more than one answer in this pack (ragged_chain.tip_inversion_ambiguous)?"""
    import ragged_chain
    pinned, olib = abi.make_pack(pack_d), oracle.load()
    for k in range(n_pops):
        first, mass, mags, tip = oracle.derive_isochrone(olib, pinned, par, k)
        if len(mass) == 0:
            continue
        for nn in node_counts:
            dM = (pack_d["m_wd_up"] - tip) / nn
            m = tip + dM * np.arange(1, nn + 1, dtype=np.float64)
            m = m[(m > tip) & (m <= pack_d["m_wd_up"])]
            prec = wd_check.wd_chain(pack_d, par, m, pop=k)[1]
            if np.any(np.abs(prec - par[abi.P_LOGAGE]) <= SEAM_TOL) or np.any(ragged_chain.tip_inversion_ambiguous(pack_d, par, k, m)):
                return False
    return True


def scripted_rows(pack_d, n_pops, node_counts, n_rows=len(TOKENS)):
    """rows [n_rows, 12]: token t of TOKENS as a row inside the cell of age index t (OUT: outside the grid, on either axis), the
    [Fe/H] cell and the place inside the cell varied by position; a place whose WD nodes fail wd_screen is moved until they pass."""
    import ragged_walk as rw
    rows = []
    for pos in range(n_rows):
        t = TOKENS[pos % len(TOKENS)]
        i_feh = (1, 2, 0)[(pos + pos // len(TOKENS)) % 3]
        if t == OUT:
            row = rw._cell_row(pack_d, 3, i_feh, 0.5)
            if pos % 2:
                row[abi.P_FEH] = pack_d["feh"][0] - 0.2
            else:
                row[abi.P_LOGAGE] = pack_d["log_age"][-1] + 1.0
            rows.append(row)
            continue
        for attempt in range(40):
            frac = (0.35, 0.6, 0.5)[pos % 3] + 0.017 * attempt * (1 if attempt % 2 else -1) + 0.0031 * (pos // len(TOKENS))
            row = rw._cell_row(pack_d, t, i_feh, min(max(frac, 0.02), 0.98))
            if wd_screen(pack_d, row, n_pops, node_counts):
                break
        else:
            raise AssertionError(f"no screened row for token {t} at position {pos}")
        rows.append(row)
    out = np.stack(rows)
    out.setflags(write=False)
    return out


def dark_pack(pack_d, eeps=(30, 31), filt=1):
    """A copy of the pack whose isochrones all give no flux (B9_MAG_NOFLUX) in filter `filt` at the EEPs `eeps`: the interpolation
    of equal corners is exact, so every derived isochrone has exactly B9_MAG_NOFLUX there and the single star's column does not
    enter."""
    d = dict(pack_d)
    nf = d["n_filt"]
    mags = np.array(d["mags"], dtype=np.float64).reshape(-1, nf).copy()
    for k in range(len(d["iso_n_eep"])):
        for e in eeps:
            i = e - int(d["iso_first_eep"][k])
            if 0 <= i < int(d["iso_n_eep"][k]):
                mags[int(d["iso_offset"][k]) + i, filt] = abi.MAG_NOFLUX
    d["mags"] = mags
    return d


class RefEngine:
    """engine.Engine.cmd_band's signature on the reference: what hostlib.cmd_band loops over in the CPU tests"""

    def __init__(self, pack_d, n_pops, mutate=None):
        self.pack_d, self.n_pops, self.mutate, self._memo = pack_d, n_pops, mutate, {}

    def _values(self, rows, spec):
        key = (np.asarray(rows).tobytes(), spec)
        if key not in self._memo:
            self._memo[key] = values(self.pack_d, rows, self.n_pops, spec, self.mutate)
        return self._memo[key]

    def cmd_band(self, rows, spec, pivot=None, mom=None, edges=None, bins=None, want_mom=True, want_bins=None):
        want_bins = edges is not None if want_bins is None else want_bins
        m, b = accumulate(self._values(rows, spec), pivot, edges if want_bins else None, mom, bins, self.mutate)
        return (m if want_mom else None), b


def order_statistic(vals, line, level):
    """(x_(ceil(a N)), a N, N) of a line: the exact order statistic a quantile bracket must contain"""
    v = np.sort(vals[:, line][~np.isnan(vals[:, line])])
    aN = level * len(v)
    return (v[max(int(math.ceil(aN)), 1) - 1] if len(v) else np.nan), aN, len(v)


def safe_edges(vals, n_bins, margin=1e-9, seed=0):
    """[n_lines, n_bins + 1] strictly ascending edges inside each line's range (so that the open words and several bins fill),
    every one more than `margin` from every value of its line: interior cuts of [min - pad, max + pad], each moved to the middle
    of the widest gap near it when a value sits too close.  A line without values gets [0, 1] cut evenly."""
    n_rows, n_lines = vals.shape
    rng = np.random.default_rng(seed)
    out = np.empty((n_lines, n_bins + 1))
    for l in range(n_lines):
        v = np.sort(vals[:, l][~np.isnan(vals[:, l])])
        if len(v) == 0:
            out[l] = np.linspace(0.0, 1.0, n_bins + 1)
            continue
        span = max(v[-1] - v[0], 1e-3 * max(1.0, abs(v[0])))
        # the first edge above the smallest value and the last below the largest where there is room: every word gets a chance
        lo, hi = v[0] + 0.13 * span * rng.uniform(0.5, 1.0), v[-1] - 0.11 * span * rng.uniform(0.5, 1.0)
        if len(v) == 1 or not hi > lo:
            lo, hi = v[0] - 0.5 * span, v[0] + 0.5 * span
        e = lo + (hi - lo) * np.arange(n_bins + 1) / max(n_bins, 1) if n_bins > 0 else np.array([lo])
        step = (hi - lo) / max(n_bins, 1)
        for b in range(n_bins + 1):
            k = 0
            while np.min(np.abs(v - e[b])) <= 10.0 * margin:
                k += 1
                e[b] += step * 1e-3 * k
                assert k < 1000
        assert np.all(np.diff(e) > 0)
        out[l] = e
    return out
