"""Small packs and the catalogue of seam cases of the WD branch ("Seams of the WD branch").

Packs: synth.make_pack / make_wd_tables shapes, edited by hand -- grid axes, every isochrone mass (so every AGB tip) and the
WD mass / carbonicity axes are snapped to dyadic values, and the rows put dyadic weights on the grid, so that the derived mass
column (first mass, tip) is EXACT in fp64 and a mass can equal a node exactly; one column of tips is flattened so that a
"not yet dead" band exists above the tip; two consecutive tips are made equal; cooling tracks of 2 and of 70 points sit side
by side; some table nodes are moved onto an anchor star's own (log cooling age, log Teff, log g).

Cases: every mass is found from the pack's numbers or by bisection on the reference (tests/wd_ref.py); none is written down.
A case is (pack, row, pop, m1, q, wd_type, family); families as in the module's CASES builder:
  a branch in mass, b precursor age, c not yet dead, d cancellation (weak), e IFMR, f cooling tracks, g atmosphere;
  cases whose reference magnitude is not a number (wd_mass <= 0) form the NaN family (weak)."""
import functools
import math

import numpy as np

import wd_ref as R
from base_amd import abi, synth


def _snap(x, bits):
    return np.round(np.asarray(x, dtype=np.float64) * 2.0 ** bits) / 2.0 ** bits


def _tracks_tables(n_carb, ragged):
    carb = _snap(np.linspace(0.2, 0.8, n_carb), 4) if n_carb > 1 else np.array([0.375])
    wmass = _snap(np.linspace(0.4, 1.2, 9), 6)

    def track(c, m, lage):
        log_teff = 5.05 - 0.27 * (lage - 6.0) - 0.012 * (lage - 6.0) ** 2 + 0.12 * (m - 0.6) + 0.05 * (c - 0.38)
        return log_teff, np.log10(8.8e8) - np.log10(m / 0.6) / 3.0 + 0.02 * (log_teff - 4.0)

    if not ragged:
        lage = _snap(np.linspace(6.0, 10.3, 24), 6)
        cc, mm, aa = np.meshgrid(carb, wmass, lage, indexing="ij")
        te, ra = track(cc, mm, aa)
        return dict(wc_carb=carb, wc_mass=wmass, wc_log_age=lage, wc_log_teff=te.ravel(), wc_log_radius=ra.ravel())
    ages, tes, ras, n_age, offset, off = [], [], [], [], [], 0
    for ic, c in enumerate(carb):
        for im, m in enumerate(wmass):
            n = 9 + 3 * ((2 * ic + im) % 5)
            if im == 4 and ic == min(1, n_carb - 1): n = 2              # a 2-point track ...
            if im == 5 and ic == min(1, n_carb - 1): n = 70             # ... next to a 70-point one
            lo, hi = 6.0 + 0.25 * ((ic + 2 * im) % 4), 10.3 - 0.6 * ((3 * ic + im) % 3)
            lage = _snap(lo + (hi - lo) * np.linspace(0.0, 1.0, n) ** (1.0 + 0.15 * (im % 3)), 10)
            te, ra = track(c, m, lage)
            ages.append(lage); tes.append(te); ras.append(ra); n_age.append(n); offset.append(off)
            off += n
    return dict(wc_carb=carb, wc_mass=wmass, wc_n_age=np.array(n_age, np.int32), wc_offset=np.array(offset, np.int64),
                wc_log_age=np.concatenate(ages), wc_log_teff=np.concatenate(tes), wc_log_radius=np.concatenate(ras))


def _pack(n_filt, n_feh, n_y, n_age, n_eep, n_carb=3, ragged=False, wd=True, n_at_type=2, teff_axis=None):
    d = synth.make_pack("parsec", n_filt, n_y=n_y, ragged=True, wd=False, n_feh=n_feh, n_age=n_age, n_eep=n_eep)
    d["log_age"], d["feh"], d["mass"] = _snap(d["log_age"], 8), _snap(d["feh"], 4), _snap(d["mass"], 24)
    if n_y > 1:
        d["y"] = _snap(d["y"], 8)
    for o, n in zip(d["iso_offset"], d["iso_n_eep"]):
        assert np.all(np.diff(d["mass"][o:o + n]) > 0)
    assert len(d["iso_n_eep"]) <= 140 and d["iso_n_eep"].max() <= 40
    if wd:
        at = synth.make_wd_tables(n_filt, n_carb=1)
        nG, nTe = len(at["at_logg"]), len(at["at_log_teff"])
        mags = at["at_mags"].reshape(2, nG, nTe, n_filt)
        if teff_axis is not None:                 # a narrower temperature axis, so that cool WDs fall below it (same rows)
            at["at_log_teff"] = np.linspace(teff_axis[0], teff_axis[1], nTe)
        d.update(_tracks_tables(n_carb, ragged))
        d.update(at_logg=at["at_logg"], at_log_teff=at["at_log_teff"], at_mags=mags[:n_at_type].copy().ravel(), n_at_type=n_at_type)
    return d


def _tip_slice(d, i_feh, i_y=0):
    nA, nY = len(d["log_age"]), len(d["y"])
    k = (i_feh * nY + i_y) * nA
    return (d["iso_offset"] + d["iso_n_eep"] - 1)[k:k + nA]


def _row(d, ia, ta, i_f, tf, iy=0, ty=0.25, **kw):
    """a parameter row with dyadic weights (ta, tf, ty) in grid cell (ia, i_f, iy)"""
    p = synth.default_params(d)
    la, fe, yy = d["log_age"], d["feh"], d["y"]
    p[abi.P_LOGAGE] = la[ia] + ta * (la[ia + 1] - la[ia])
    p[abi.P_FEH] = fe[i_f] + tf * (fe[i_f + 1] - fe[i_f])
    if len(yy) > 1:
        p[abi.P_Y] = yy[iy] + ty * (yy[iy + 1] - yy[iy])
        p[abi.P_Y2] = yy[-2] + 0.5 * (yy[-1] - yy[-2])
    p[abi.P_CARBONICITY] = 0.375
    for k, v in kw.items():
        p[getattr(abi, "P_" + k.upper())] = v
    return p


@functools.lru_cache(maxsize=None)
def packs():
    """name -> (pack dict, list of rows).  Built once; the anchor edits need the reference."""
    out = {}
    # A: rectangular tracks, carbonicity axis, 8 filters, n_age = 9 (one round of the 8-ary search), n_y = 1
    a = _pack(8, 4, 1, 9, 40, n_carb=3, ragged=False)
    t2 = _tip_slice(a, 2)
    a["mass"][t2] = _snap(0.7 * a["mass"][t2] + 0.3 * a["mass"][t2][0], 24)    # flatter, larger tips at FeH node 2: the not-yet-dead band
    t1 = _tip_slice(a, 1)
    a["mass"][t1[3]] = a["mass"][t1[2]]                                        # two equal consecutive tips at FeH node 1
    a["mass"][t2[2]] = a["mass"][t1[1]]                                        # one mass on a tip of BOTH columns (see row 7)
    assert a["mass"][t2[1]] > a["mass"][t2[2]] > a["mass"][t2[3]]
    rows_a = [_row(a, 5, 0.25, 1, 0.5),                                        # 0: the default row
              _row(a, 7, 0.875, 1, 0.5),                                       # 1: last age cell (a corner can be light)
              _row(a, 0, 0.25, 1, 0.5),                                        # 2: first age cell (every corner heavy just above the tip)
              _row(a, 5, 0.25, 1, 0.5, carbonicity=0.125),                     # 3-5: carbonicity below, on, above its axis
              _row(a, 5, 0.25, 1, 0.5, carbonicity=0.5),
              _row(a, 5, 0.25, 1, 0.5, carbonicity=0.9375),
              _row(a, 4, 0.25, 0, 0.5),                                        # 6: cell without the flattened column
              _row(a, 1, 0.5, 1, 0.5)]                                         # 7: logAge = (log_age[1] + log_age[2]) / 2: prec == logAge EXACTLY at that mass
    _anchor(a, rows_a[0])
    a["d_row0"] = _cancellation_rows(a, rows_a, *D_SITES["A"])                 # 8-12: family d
    out["A"] = (a, rows_a)
    for nm, iid in (("Aw", abi.IFMR_WEIDEMANN), ("As", abi.IFMR_SALARIS_LIN), ("Ap", abi.IFMR_SALARIS_PW)):
        out[nm] = (dict(a, ifmr_id=iid), [_row(a, 6, 0.5, 1, 0.5), _row(a, 2, 0.5, 1, 0.5), _row(a, 7, 0.875, 0, 0.5)])
    wm = a["wc_mass"]
    lin = [dict(ifmr_intercept=v, ifmr_slope=0.125, ifmr_quad=0.0078125) for v in
           (0.25, float(wm[3]), 1.5, 2.0 ** -30, 0.0, -0.25, 8.0)]           # wd_mass at m = 3: below, node, above, tiny, 0, < 0, huge
    out["Al"] = (dict(a, ifmr_id=abi.IFMR_LINEAR), [_row(a, 5, 0.25, 1, 0.5, **k) for k in lin])
    # B: ragged tracks (2 points next to 70), helium axis (n_y = 3), 5 filters, n_age = 8 (tail only), quadratic IFMR
    b = _pack(5, 3, 3, 8, 30, n_carb=3, ragged=True, teff_axis=(4.1, 4.6))
    b["ifmr_id"] = abi.IFMR_QUADRATIC
    rows_b = [_row(b, 4, 0.25, 0, 0.5, 0, 0.25), _row(b, 6, 0.875, 1, 0.25, 1, 0.5), _row(b, 0, 0.5, 0, 0.5, 0, 0.75)] + \
             [_row(b, 4, 0.25, 0, 0.5, 0, 0.25, **k) for k in lin] + \
             [_row(b, 4, 0.25, 0, 0.5, 0, 0.25, carbonicity=c) for c in (0.125, 0.5, 0.9375)]
    out["B"] = (b, rows_b)
    # C: no carbonicity axis, ragged tracks, DA atmospheres only, 3 filters, n_age = 65 (two rounds)
    c = _pack(3, 2, 1, 65, 20, n_carb=1, ragged=True, n_at_type=1)
    rows_c = [_row(c, 40, 0.25, 0, 0.5), _row(c, 63, 0.875, 0, 0.25), _row(c, 0, 0.5, 0, 0.5)]
    c["d_row0"] = _cancellation_rows(c, rows_c, *D_SITES["C"])                 # 3-7: family d
    out["C"] = (c, rows_c)
    # D: no WD tables
    d = _pack(3, 3, 1, 8, 20, wd=False)
    out["D"] = (d, [_row(d, 4, 0.25, 1, 0.5)])
    return out


def _anchor(d, row):
    """Move one node of the shared cooling-age axis, of the log Teff axis and of the log g axis onto the values of an anchor
    star (m = midway between the tip and M_wd_up), so that its lookups are ON a node to within a rounding."""
    md = R.Model(R.REF, d, row)
    m = float(np.float32(0.5 * (float(md.tip.v) + d["m_wd_up"])))
    d["anchor_mass"] = m
    for key, q in (("wc_log_age", "log_cool"), ("at_log_teff", "log_teff"), ("at_logg", "logg")):
        r = R.evaluate(d, row, 0, m, 0.0, 0)
        x = float(r[q].v)
        ax = d[key]
        j = int(np.argmin(np.abs(ax[1:-1] - x))) + 1
        assert ax[j - 1] < x < ax[j + 1]
        ax[j] = x


@functools.lru_cache(maxsize=None)
def model(name, irow, pop=0):
    d, rows = packs()[name]
    return R.Model(R.REF, d, rows[irow], pop)


def ref(name, irow, pop, m1, q, wd_type, **kw):
    d, rows = packs()[name]
    return R.evaluate(d, rows[irow], pop, m1, q, wd_type, model=model(name, irow, pop), **kw)


def first_true(pred, lo, hi):
    """The smallest fp64 in (lo, hi] at which the monotone predicate holds (pred(lo) false, pred(hi) true): bisection on the
    doubles themselves, so the answer and its predecessor are neighbours."""
    assert not pred(lo) and pred(hi)
    while math.nextafter(lo, math.inf) < hi:
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            mid = math.nextafter(lo, math.inf)
        if pred(mid): hi = mid
        else: lo = mid
    return hi


def meets_budget(r, weak_ok=False):
    """the condition of the non-weak families: kappa u <= 2^-10 and every budget <= 1e-9 max(1, |value|)"""
    if r.get("kappa") is not None and not r["kappa"] * float(R.U) <= 2.0 ** -10:
        return False
    for x in list(r.get("app_mags") or []) + [r.get(k) for k in ("prec", "wd_mass", "log_cool", "log_teff", "logg")]:
        if isinstance(x, R.V) and not float(x.e) <= 1e-9 * max(1.0, abs(float(x.v))):
            return False
    return True


def _up(x, k=1):
    for _ in range(k): x = math.nextafter(x, math.inf)
    return x


def _dn(x, k=1):
    for _ in range(k): x = math.nextafter(x, -math.inf)
    return x


@functools.lru_cache(maxsize=None)
def cases():
    """The catalogue: a list of dicts (pack, row, pop, m1, q, wd_type, fam)."""
    P = packs()
    out = []

    def add(fam, pack, row, m1, q=0.0, wd_type=0, pop=0):
        out.append(dict(fam=fam, pack=pack, row=row, pop=pop, m1=float(m1), q=float(q), wd_type=int(wd_type)))

    def chain(pack, row, m):                       # the chain up to log_cool only (what the bisections look at)
        o = {}
        return model(pack, row).wd_chain(float(m), set(), o, stop="log_cool"), o

    def lc(pack, row, m):
        st, o = chain(pack, row, m)
        return float(o["log_cool"].v) if st == R.WD else -math.inf

    def well(pack, row, m):                        # a live WD whose log_cool is well inside the budget condition
        st, o = chain(pack, row, m)
        return st == R.WD and o["kappa"] * float(R.U) <= 2.0 ** -10 and float(o["log_cool"].e) <= 1e-11

    for name, (d, rows) in P.items():
        up = float(d["m_wd_up"])
        for irow in range(min(len(rows), d.get("d_row0", len(rows)))):        # (the family-d rows have their own builder)
            md = model(name, irow)
            tip, first = float(md.tip.v), float(md.mass[0].v)
            mf = R.Model(R.F64, d, rows[irow])
            assert mf.tip == md.tip.v and mf.mass[0] == md.mass[0].v, "the derived tip and first mass must be exact in fp64"
            # a. branch in mass: one ulp either side of and on the first mass, the tip, M_wd_up; mixed and dark systems
            if irow < 3:
                for x in (first, tip, up):
                    for m in (_dn(x), x, _up(x)):
                        add("a", name, irow, m, wd_type=irow & 1)
                add("a", name, irow, 0.5 * (tip + up), q=0.5 * tip / (0.5 * (tip + up)))          # WD primary, MS companion
                add("a", name, irow, _up(up), q=0.5 * first / up)                                 # NS/BH + below the first mass: dark
                add("a", name, irow, 0.0); add("a", name, irow, -1.0)
            if not md.has_wd:
                continue
            # b. precursor age: on the corner columns' tips 0, 1, na-2, na-1, between the tips[0] of the corners, above all of them
            if irow < 3:
                t0s = sorted(t[0] for t in md.tips.values())
                for t in md.tips.values():
                    for j in (0, 1, len(t) - 2, len(t) - 1):
                        if tip < t[j] <= up: add("b", name, irow, t[j])
                    for j in range(len(t) - 1):
                        if t[j] == t[j + 1] and tip < t[j] <= up:
                            add("b", name, irow, t[j]); add("b", name, irow, _dn(t[j])); add("b", name, irow, _up(t[j]))
                    if tip < t[-1]:                                            # light at this corner (and not at a corner with smaller tips)
                        add("b", name, irow, 0.5 * (tip + t[-1])); add("b", name, irow, t[-1]); add("b", name, irow, _up(t[-1]))
                if t0s[0] < t0s[-1] and t0s[-1] <= up:
                    add("b", name, irow, 0.5 * (max(tip, t0s[0]) + t0s[-1]))   # heavy at one corner only
                if t0s[-1] < up:
                    add("b", name, irow, 0.5 * (max(tip, t0s[-1]) + up), wd_type=1)   # heavy at every corner
            # c. not yet dead: where the band exists, the last dead mass and the first live one that meets the budget condition
            alive = lambda m: chain(name, irow, m)[0] == R.WD
            if irow < 3 and not alive(_up(tip)) and alive(up):
                m_live = first_true(alive, _up(tip), up)
                la = rows[irow][abi.P_LOGAGE]
                dead_sure = lambda m: not ((pr := chain(name, irow, m)[1]["prec"]).v - la > R.tolerance(pr))
                add("c", name, irow, _dn(first_true(dead_sure, _up(tip), m_live)))
                add("c", name, irow, 0.5 * (tip + m_live))
                add("c", name, irow, first_true(lambda m: well(name, irow, m), _dn(m_live), up))
            # f. cooling tracks: log_cool at a node of, below the first and above the last point of the neighbouring tracks
            if irow in F_ROWS.get(name, (0,)):
                lo_m = first_true(lambda m: well(name, irow, m), tip, up)
                tr = md.tracks
                ends = sorted({t[0][0] for t in tr} | {t[0][-1] for t in tr})
                targets = [0.5 * (x + y) for x, y in zip(ends, ends[1:])] + [max(tr, key=lambda t: len(t[0]))[0][3]]
                lc_lo, lc_up = lc(name, irow, lo_m), lc(name, irow, up)
                for TT in targets:                                             # between the ends of different tracks; on a node
                    if lc_lo < TT <= lc_up:
                        m = first_true(lambda m: lc(name, irow, m) >= TT, lo_m, up)
                        add("f", name, irow, m, wd_type=len(out) & 1); add("f", name, irow, _dn(m))
                for k in range(1, 12):                                         # a ladder through the WD mass axis (every pair of tracks)
                    add("f", name, irow, lo_m + (up - lo_m) * k / 12.0, wd_type=k & 1)
                if "anchor_mass" in d and irow == 0:
                    add("f", name, 0, d["anchor_mass"]); add("g", name, 0, d["anchor_mass"], wd_type=1)
                # g. atmosphere: the hottest (just above the tip) and coolest WDs of the row, DA and DB
                for m in (lo_m, _up(lo_m, 3), up, _dn(up)):
                    add("g", name, irow, m, wd_type=0); add("g", name, irow, m, wd_type=1)
        # d. cancellation: prec is a grid age EXACTLY (m on a tip of a row that sits on a FeH node), logAge k ulps above it
        # e. IFMR
        if name in ("Aw", "As", "Ap"):
            for irow in range(len(rows)):
                tip = float(model(name, irow).tip.v)
                for m in [float(k) for k in range(1, 8)] + [0.9375, 7.5, _dn(4.0), _up(4.0), 2.5, 5.25]:
                    if tip < m <= up: add("e", name, irow, m)
        if name in ("Al", "B"):
            for irow in range(len(rows)):
                tip = float(model(name, irow).tip.v)
                for m in (3.0, 3.5, 0.5 * (tip + 3.0), 6.0):
                    if tip < m <= up: add("e", name, irow, m, wd_type=irow & 1)
    a, _ = P["A"]                                    # c, exactly ON the seam: prec == logAge above the tip (row 7 of pack A)
    T = float(a["mass"][_tip_slice(a, 1)[1]])
    for m in (_dn(T), T):                            # (one ulp above T the star lives at kappa ~ 1e16: not a decidable case)
        add("c", "A", 7, m)
    out += _cancellation()
    for c in out:
        c["ref"] = ref(c["pack"], c["row"], c["pop"], c["m1"], c["q"], c["wd_type"])
        if any(a == "nan" for a in (c["ref"].get("app_mags") or [])):
            c["fam"] = "NaN"
    return out


D_ULPS = (1, 2, 16, 1000, 10 ** 6)
D_SITES = {"A": (1, 5), "C": (0, 40)}            # family d: pack -> (FeH node the row sits on, tip index the mass sits on)


def _cancellation_rows(d, rows, i_f, j):
    """Family d, appended to a pack's rows by packs(): the row sits ON FeH node i_f (weight 0: prec is the lower corner's value
    exactly) and logAge = log_age[j] + k ulps, k in D_ULPS; a mass ON that column's tip j has prec = log_age[j] exactly, in
    every implementation.  Returns the index of the first of these rows."""
    first = len(rows)
    la = float(d["log_age"][j])
    for k in D_ULPS:
        p = _row(d, j, 0.0, i_f, 0.0)
        p[abi.P_LOGAGE] = la + k * math.ulp(la)
        rows.append(p)
    return first


def _cancellation():
    out = []
    for name, (i_f, j) in D_SITES.items():
        d, rows = packs()[name]
        tips = d["mass"][_tip_slice(d, i_f)]
        for n, k in enumerate(D_ULPS):
            out.append(dict(fam="d", pack=name, row=d["d_row0"] + n, pop=0, m1=float(tips[j]), q=0.0, wd_type=k & 1, ulps=k))
    return out


WEAK = ("d", "NaN")
F_ROWS = {"A": (0, 3, 4, 5), "B": (0, 10, 11, 12)}      # the rows whose cooling-track and atmosphere ladders are built


def catalogue(name, prior=1.0, sigma=0.03125, pop=None):
    """The cases of one pack as star catalogues, one per parameter row (a case belongs to its row): {row index: (cluster dict,
    [case, ...])} -- obs = the reference's magnitudes + known offsets; cases with m1 <= 0 are no catalogue entries."""
    d, rows = packs()[name]
    nf = d["n_filt"]
    by_row = {}
    for c in cases():
        if c["pack"] == name and c["m1"] > 0.0 and (pop is None or c["pop"] == pop):
            by_row.setdefault(c["row"], []).append(c)
    out = {}
    for irow, cs in by_row.items():
        obs = np.empty((len(cs), nf))
        for i, c in enumerate(cs):
            obs[i] = case_obs(d, rows[irow], c)
        out[irow] = (cluster_of(d, cs, obs, sigma, prior), cs)
    return out


OFFSETS = np.array([0.03125, -0.015625, 0.046875, -0.0078125, 0.0234375, -0.0390625, 0.01171875, -0.02734375])


def case_obs(d, row, c):
    """the reference's predicted magnitudes (as the likelihood sees them) + the known offsets; 20 where it is not a number"""
    return np.array([(20.0 if isinstance(a, str) else float(a.v)) + OFFSETS[f] for f, a in enumerate(c["ref"]["like_mags"])])


def cluster_of(d, cs, obs, sigma, prior):
    n, nf = len(cs), d["n_filt"]
    return dict(n_filt=nf, obs=np.ascontiguousarray(obs), sigma=np.full((n, nf), float(sigma)),
                mass1=np.array([c["m1"] for c in cs]), mass_ratio=np.array([c["q"] for c in cs]),
                clust_prior=np.full(n, float(prior)), stage=np.full(n, abi.STAGE_WD, np.int32),
                wd_type=np.array([c["wd_type"] for c in cs], np.int32),
                filter_prior_min=np.full(nf, -8.0), filter_prior_max=np.full(nf, 120.0))


LOG_FS = lambda nf: -nf * math.log(128.0)


def like(name, c, sigma, prior):
    """the reference's per-star value of case c observed at case_obs: dict(c0, ll, value) of wd_ref.loglike"""
    d, rows = packs()[name]
    nf = d["n_filt"]
    return R.loglike(R.REF, d, c["ref"], c["m1"], case_obs(d, rows[c["row"]], c), np.full(nf, float(sigma)), prior, LOG_FS(nf))


def mag_ratio(c, got):
    """max over the filters of |got - reference| / tolerance for apparent magnitudes `got` of case c; a filter without flux must
    be exactly B9_MAG_NOFLUX, one that is not a number must not be finite (inf then)."""
    worst = 0.0
    for a, g in zip(c["ref"]["app_mags"], got):
        if a is None:
            worst = max(worst, 0.0 if g == abi.MAG_NOFLUX else math.inf)
        elif isinstance(a, str):
            worst = max(worst, math.inf if math.isfinite(g) else 0.0)
        elif not math.isfinite(g):
            worst = math.inf
        else:
            worst = max(worst, abs(float(R.M.mpf(float(g)) - a.v)) / R.tolerance(a))
    return worst


def value_ratio(x, got):
    """|got - reference| / tolerance for a value of wd_ref.loglike (None = -inf)"""
    if x is None:
        return 0.0 if got == -math.inf else math.inf
    if not math.isfinite(got):
        return math.inf
    return abs(float(R.M.mpf(float(got)) - x.v)) / R.tolerance(x)
