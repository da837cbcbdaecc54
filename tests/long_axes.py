"""Grid axes of real model-set length (64 .. 513 entries): the packs, the positions beside the bracket's regime boundaries, an
exact statement of DESIGN.md section 2's isochrone, an emulation of the device's counting bracket with its mutants, and the
scripted chains, shared by tests/test_long_axes_host.py (CPU) and tests/test_gpu_long_axes.py (GPU).  Nothing here needs a GPU.

Packs: synth.make_pack(..., ragged=True) shapes built vectorised (the largest has 16 641 isochrones), small everywhere except
the axis under test; axes and masses are snapped to dyadic values and every isochrone ends ON its analytic AGB tip, so that
every tip column descends strictly along the age axis however fine that axis is.

Bracket: the largest i <= n - 2 with ax[i] <= x.  The device finds it by counting (b9_derive.hip.h) in
one of three regimes: n <= 64 (one register of axis values per lane, the second all padding), 65 .. 128 (two registers), and
> 128 (the axis walked in memory in 64-entry chunks)."""
import collections
import functools
import math

import numpy as np

import wd_ref as R
import wd_seams as S
from base_amd import abi, mcmc, synth

AGE_BITS, FEH_BITS, Y_BITS, MASS_BITS = 16, 12, 16, 24
NODES = (0, 1, 62, 63, 64, 65, 126, 127, 128, 129, 191, 192, 193)

#: name -> (filters, n_feh, n_y, n_age, EEPs, WD tables as tests/wd_seams.py snaps them, axes under test)
SHAPES = collections.OrderedDict([
    ("a64", (3, 2, 1, 64, 12, False, "a")), ("a65", (3, 2, 1, 65, 12, False, "a")), ("a127", (3, 2, 1, 127, 12, False, "a")),
    ("a128", (4, 2, 1, 128, 12, False, "a")), ("a129", (3, 2, 1, 129, 12, False, "a")), ("a193", (3, 2, 1, 193, 12, False, "a")),
    ("a513", (3, 2, 1, 513, 8, False, "a")),
    ("f129", (4, 129, 1, 2, 8, False, "f")), ("y129", (3, 2, 129, 2, 8, False, "y")), ("af129", (3, 129, 1, 129, 8, False, "af")),
    ("w17x129", (3, 17, 1, 129, 12, True, "a")),       # 2193 tips: corner columns, two rounds of the 8-ary search
    ("w3x3x513", (5, 3, 3, 513, 8, True, "a")),        # 4617 tips: corner columns, three rounds; two populations
    ("w513", (3, 2, 1, 513, 8, True, "a")),            # 1026 tips: staged whole, three rounds
])
AXIS_KEY = {"a": ("log_age", abi.P_LOGAGE), "f": ("feh", abi.P_FEH), "y": ("y", abi.P_Y)}


def grid_pack(n_filt, n_feh, n_y, n_age, n_eep, wd_snapped=False):
    """synth.make_pack("parsec", ragged=True)'s isochrones on dyadic axes of any length, without its per-isochrone loop."""
    feh = S._snap(np.linspace(-2.0, 0.5, n_feh), FEH_BITS)
    log_age = S._snap(np.linspace(7.8, 10.2, n_age), AGE_BITS)
    y = np.array([0.27]) if n_y == 1 else S._snap(np.linspace(0.23, 0.35, n_y), Y_BITS)
    for ax in (feh, log_age, y):
        assert np.all(np.diff(ax) > 0), "an axis must stay strictly ascending after the snap"
    i_f, i_y, i_a = (x.ravel() for x in np.meshgrid(np.arange(n_feh), np.arange(n_y), np.arange(n_age), indexing="ij"))
    first = ((i_f + 2 * i_a + i_y) % 3).astype(np.int32)
    count = (n_eep - first - (3 * i_f + i_a) % 4).astype(np.int32)
    offset = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64)
    iso = np.repeat(np.arange(len(count)), count)
    ids = (np.arange(count.sum()) - offset[iso] + first[iso]).astype(np.float64)
    la_p, fe_p, y_p = log_age[i_a][iso], feh[i_f][iso], y[i_y][iso]
    mass, mags = synth._iso_points(la_p, fe_p, y_p, ids, n_eep, n_filt)
    last = offset + count - 1
    mass[last] = synth._iso_points(log_age[i_a], feh[i_f], y[i_y], np.full(len(count), n_eep - 1.0), n_eep, n_filt)[0]
    mass = S._snap(mass, MASS_BITS)
    inner = np.ones(len(mass), bool)
    inner[offset] = False
    assert np.all(np.diff(mass)[inner[1:]] > 0), "every mass column strictly ascending"
    assert np.all(np.diff(mass[last].reshape(n_feh * n_y, n_age), axis=1) < 0), "every tip column strictly descending"
    d = dict(name="long", n_filt=n_filt, feh=feh, y=y, log_age=log_age, iso_first_eep=first, iso_n_eep=count, iso_offset=offset,
             mass=mass, mags=np.ascontiguousarray(mags), abs_coeff=synth.ABS_COEFF_8[:n_filt].copy(),
             filters=synth.FILTERS_8[:n_filt], ifmr_id=abi.IFMR_WILLIAMS, m_wd_up=8.0)
    at = synth.make_wd_tables(n_filt, n_carb=1)
    if wd_snapped:
        d.update(S._tracks_tables(1, True))
        d.update(at_logg=at["at_logg"], at_log_teff=at["at_log_teff"], at_mags=at["at_mags"], n_at_type=2)
    else:
        d.update(at)
    return d


@functools.lru_cache(maxsize=None)
def pack(name):
    nf, n_feh, n_y, n_age, n_eep, wd, _ = SHAPES[name]
    return grid_pack(nf, n_feh, n_y, n_age, n_eep, wd)


# ---- positions ---------------------------------------------------------------------------------------------------------------
def bracket(ax, x):
    """DESIGN.md section 2, as it is written: the largest i <= n - 2 with ax[i] <= x (0 where there is none)"""
    i = 0
    for k in range(len(ax) - 1):
        if ax[k] <= x:
            i = k
    return i


def base_row(d):
    """every axis at a dyadic interior weight of an interior cell (the middle one)"""
    la, fe, yy = d["log_age"], d["feh"], d["y"]
    ia, i_f, iy = (len(la) - 1) // 2, (len(fe) - 1) // 2, (len(yy) - 1) // 2
    p = S._row(d, ia, 0.25, i_f, 0.5, iy, 0.25)
    p[abi.P_MOD], p[abi.P_ABS] = 0.0, 0.0
    return p


Position = collections.namedtuple("Position", "axis node kind x cell row")


@functools.lru_cache(maxsize=None)
def positions(name):
    """The positions of a pack: per axis under test and node j of NODES + the last three, x on ax[j], one ulp either side and
    midway to ax[j + 1]; cell = the expected bracket on that axis, None where x is outside the grid (one ulp below ax[0], one
    above ax[n - 1])."""
    d, out = pack(name), []
    for a in SHAPES[name][6]:
        key, col = AXIS_KEY[a]
        ax = [float(v) for v in d[key]]
        n = len(ax)
        for j in sorted({k for k in NODES + (n - 3, n - 2, n - 1) if 0 <= k < n}):
            for kind, x in (("below", math.nextafter(ax[j], -math.inf)), ("on", ax[j]), ("above", math.nextafter(ax[j], math.inf)),
                            ("mid", 0.5 * (ax[j] + ax[j + 1]) if j + 1 < n else None)):
                if x is None:
                    continue
                row = base_row(d)
                row[col] = x
                out.append(Position(a, j, kind, x, bracket(ax, x) if ax[0] <= x <= ax[-1] else None, row))
    return out


# ---- the reference isochrone ---------------------------------------------------------------------------------------------------
def lerp(a, b, t):
    return R._fma(t, b - a, a)


Iso = collections.namedtuple("Iso", "first n mass mags tip cell t")


def derive(d, row, pop=0, cell=None):
    """DESIGN.md section 2's isochrone of a parameter row, exactly: bracket as above, t = (x - ax[i]) / (ax[i + 1] - ax[i]) in
    fp64, every value three nested lerps (age, then Y where it is an axis, then FeH), lerp(a, b, t) = fma(t, b - a, a) with
    b - a rounded and the fma exact (wd_ref._fma); the EEP range is the corners' intersection; the tip the last mass.  None
    where the row lies outside the grid or fewer than two EEPs are common.  cell: brackets to use instead (extrapolating)."""
    axes = [[float(v) for v in d[k]] for k in ("log_age", "feh", "y")]
    x = [float(row[abi.P_LOGAGE]), float(row[abi.P_FEH]), float(row[abi.P_Y2 if pop else abi.P_Y])]
    nA, nY, nf = len(axes[0]), len(axes[2]), int(d["n_filt"])
    ny = 2 if nY > 1 else 1
    for k in range(3 if ny == 2 else 2):
        if not axes[k][0] <= x[k] <= axes[k][-1]:
            return None
    if cell is None:
        cell = (bracket(axes[0], x[0]), bracket(axes[1], x[1]), bracket(axes[2], x[2]) if ny == 2 else 0)
    t = [(x[k] - axes[k][i]) / (axes[k][i + 1] - axes[k][i]) if (k < 2 or ny == 2) else 0.0 for k, i in enumerate(cell)]
    ia, i_f, iy = cell
    ks = {(df, dy, da): ((i_f + df) * nY + iy + dy) * nA + ia + da for df in range(2) for dy in range(ny) for da in range(2)}
    first, cnt, off = d["iso_first_eep"], d["iso_n_eep"], d["iso_offset"]
    lo = max(int(first[k]) for k in ks.values())
    n = min(int(first[k]) + int(cnt[k]) for k in ks.values()) - lo
    if n < 2:
        return None
    pt = {c: int(off[k]) + lo - int(first[k]) for c, k in ks.items()}
    mass_t, mags_t = d["mass"], np.asarray(d["mags"]).reshape(-1, nf)

    def value(e, f):
        v = lambda c: float(mass_t[pt[c] + e] if f is None else mags_t[pt[c] + e, f])
        vf = []
        for df in range(2):
            vy = [lerp(v((df, dy, 0)), v((df, dy, 1)), t[0]) for dy in range(ny)]
            vf.append(lerp(vy[0], vy[1], t[2]) if ny == 2 else vy[0])
        return lerp(vf[0], vf[1], t[1])

    mass = np.array([value(e, None) for e in range(n)])
    mags = np.array([[value(e, f) for f in range(nf)] for e in range(n)])
    return Iso(lo, n, mass, mags, float(mass[-1]), cell, tuple(t))


@functools.lru_cache(maxsize=None)
def reference(name, k, pop=0):
    return derive(pack(name), positions(name)[k].row, pop)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_isochrone(want, got):
    """got = (first_eep, mass, mags, tip) of Engine.derive_isochrone / oracle.derive_isochrone: bit for bit the reference's,
    empty where the reference has none.  Returns the number of doubles compared."""
    first, mass, mags, tip = got
    if want is None:
        assert len(mass) == 0 and mags.size == 0, (first, len(mass))
        return 0
    assert first == want.first and len(mass) == want.n, (first, len(mass), want.first, want.n)
    assert same_bits(mass, want.mass), np.flatnonzero(mass != want.mass)
    assert same_bits(mags, want.mags), np.argwhere(mags != want.mags)[:4]
    assert same_bits([tip], [want.tip])
    return mass.size + mags.size + 1


def ulps_apart(a, b):
    """the largest distance of two equally shaped fp64 arrays in units of the larger value's ulp"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))))


def cell_sensitivity(name, k):
    """{-1, +1 -> what moving the bracket of position k's axis by one cell does to the derived isochrone: None where that cell
    does not exist, else the largest change of a derived value in ulps (inf where the EEP range changes)}"""
    d, p = pack(name), positions(name)[k]
    want = reference(name, k)
    n = len(d[AXIS_KEY[p.axis][0]])
    ai = "afy".index(p.axis)
    out = {}
    for step in (-1, 1):
        c = list(want.cell)
        c[ai] += step
        if not 0 <= c[ai] <= n - 2:
            out[step] = None
            continue
        moved = derive(d, p.row, 0, tuple(c))
        if moved is None or (moved.first, moved.n) != (want.first, want.n):
            out[step] = math.inf
        else:
            out[step] = max(ulps_apart(moved.mass, want.mass), ulps_apart(moved.mags, want.mags))
    return out


# ---- the device's counting bracket, emulated ---------------------------------------------------------------------------------------
MUTANTS = ("lt_for_le", "second_register_dropped", "registers_beyond_128", "last_chunk_unmasked", "padding_zero", "clamp_n_minus_1",
           "chunk_stride_63")


def device_bracket(ax, x, mutant=None):
    """b9_derive.hip.h's bracket_regs / bracket_wave, lane by lane: lane l holds ax[l] and ax[l + 64] (+inf where the axis has
    ended) and the bracket is the popcount of the two ballots of `<= x`, less one; beyond 128 entries the axis is walked in
    memory, 64 entries a chunk, the lanes past the end of the last chunk masked out; the result is clamped to [0, n - 2].
    An unmasked lane reads what lies behind the axis, taken here to be 0.0."""
    n = len(ax)
    le = (lambda v: v < x) if mutant == "lt_for_le" else (lambda v: v <= x)
    pad = 0.0 if mutant == "padding_zero" else math.inf
    if n <= 128 or mutant == "registers_beyond_128":
        v0 = [ax[l] if l < n else pad for l in range(64)]
        v1 = [ax[l + 64] if l + 64 < n else pad for l in range(64)]
        cnt = sum(map(le, v0)) + (0 if mutant == "second_register_dropped" else sum(map(le, v1)))
    else:
        cnt = 0
        for base in range(0, n, 63 if mutant == "chunk_stride_63" else 64):
            for lane in range(64):
                j = base + lane
                if j < n:
                    cnt += le(ax[j])
                elif mutant == "last_chunk_unmasked":
                    cnt += le(0.0)
    i = cnt - 1
    return max(0, min(i, n - 1 if mutant == "clamp_n_minus_1" else n - 2))


# ---- R2: stars ON the nodes of a row's own mass column -----------------------------------------------------------------------------
def node_stars(d, iso, n_stars=64, sigma=2.0 ** -40):
    """(cluster dict, c0[n_stars]): single MS stars whose masses are the derived mass column's own entries (star k on EEP
    k mod (n - 1): never the last, whose weight in its bracket is 1, not 0) observed at the reference's magnitudes there --
    the star's weight in its mass bracket is 0 and the row's modulus and absorption are 0, so its magnitudes are the derived
    ones whatever the order of the remaining operations.  c0: the star's constant (mass prior + Gaussian constants,
    wd_ref.loglike)."""
    nf = int(d["n_filt"])
    e = np.arange(n_stars) % (iso.n - 1)
    obs = iso.mags[e].copy()
    cs = [dict(m1=float(iso.mass[i]), q=0.0, wd_type=0) for i in e]
    cl = S.cluster_of(d, cs, obs, sigma, 1.0)
    cl["stage"] = np.full(n_stars, abi.STAGE_MSRG, np.int32)
    sig = np.full(nf, sigma)
    c0 = {}
    for i in set(e.tolist()):
        c0[i] = float(R.loglike(R.F64, d, dict(app_mags=[0.0] * nf, like_mags=[float(v) for v in obs[i]]), float(iso.mass[i]), obs[i], sig,
                                1.0, None)["c0"])
    return cl, np.array([c0[i] for i in e.tolist()])


# ---- R3: the scripted chains ---------------------------------------------------------------------------------------------------
#: A script: 8 walkers, 16 steps, proposal steps of about one cell width on the long axes.  The catalogue is drawn midway
#: between the two boundaries with its errors widened (ragged_walk.catalogue) until a step of one cell costs about one unit of
#: log-posterior: proposals across a boundary are then accepted and rejected in both directions.  boundaries: cell-index
#: thresholds b -- a proposal crosses b when the bracket moves between <= b - 1 and >= b.  Index 63|64 is threshold 64 (entry
#: 64, the first of the second register, starts to count); index 127|128 is threshold 128 where the axis has 130 entries or more
#: and 127 on the 129-entry axes, whose entry 128 is the grid's last: there the walker enters and leaves the cell [ax[127], ax[128]].
Script = collections.namedtuple("Script", "name pack mode n_pops K Q seed sigma_scale step")
GIVEN, MARG = abi.MODE_GIVEN_MASS, abi.MODE_MARGINALISED
WALKERS, STEPS, N_STARS = 8, 16, 120
SCRIPTS = [
    Script("a129-g1", "a129", GIVEN, 1, 0, 0, 12, 40.0, 1.0), Script("a129-g2", "a129", GIVEN, 2, 0, 0, 39, 80.0, 1.0),
    Script("a129-m1", "a129", MARG, 1, 1, 2, 70, 30.0, 1.0),
    Script("a193-g1", "a193", GIVEN, 1, 0, 0, 44, 20.0, 1.0), Script("a193-g2", "a193", GIVEN, 2, 0, 0, 6, 40.0, 0.7),
    Script("a193-m1", "a193", MARG, 1, 1, 2, 16, 20.0, 1.0),
    Script("af129-g1", "af129", GIVEN, 1, 0, 0, 52, 40.0, 1.0), Script("af129-g2", "af129", GIVEN, 2, 0, 0, 1, 40.0, 1.0),
    Script("af129-m1", "af129", MARG, 1, 1, 2, 44, 40.0, 1.0),
]


def thresholds(n):
    return {"63|64": 64, "127|128": 128 if n >= 130 else 127}


_BUILT = {}


def build_script(sc):
    """dict(pack_d, cl, pack, stars, priors, options, start, free, chol, ids, axes) of a script; built once and left unchanged"""
    import ragged_walk as rw
    if sc.name not in _BUILT:
        d = pack(sc.pack)
        la, fe = d["log_age"], d["feh"]
        long_feh = len(fe) > 64
        truth = S._row(d, 96, 0.25, 96 if long_feh else 0, 0.5)
        truth[abi.P_MOD], truth[abi.P_ABS] = 10.2, 0.12
        cl = rw.catalogue(d, truth, N_STARS, sc.seed, 0.05, sc.n_pops, sigma_scale=sc.sigma_scale)
        th = thresholds(len(la))
        rng = np.random.default_rng(sc.seed + 7)
        start = np.tile(truth, (WALKERS, 1))
        for w in range(WALKERS):
            b = th["63|64"] if w % 2 == 0 else th["127|128"]
            start[w, abi.P_LOGAGE] = la[b] + (la[b + 1 if b + 1 < len(la) else b] - la[b - 1]) * 0.5 * rng.uniform(-0.6, 0.6)
            start[w, abi.P_LOGAGE] = min(start[w, abi.P_LOGAGE], la[-1] - 0.1 * (la[-1] - la[-2]))
            if long_feh:
                b = th["63|64"] if (w // 2) % 2 == 0 else th["127|128"]
                start[w, abi.P_FEH] = fe[b] + (fe[b] - fe[b - 1]) * rng.uniform(-0.6, 0.0 if b + 1 == len(fe) else 0.6)
        free = [abi.P_LOGAGE, abi.P_FEH, abi.P_MOD, abi.P_ABS] + ([abi.P_LAMBDA] if sc.n_pops == 2 else [])
        da, df = float(la[1] - la[0]), float(fe[1] - fe[0]) if long_feh else 2e-3
        chol = np.diag([da * sc.step, df * sc.step, 2e-3, 1e-3] + ([2e-2] if sc.n_pops == 2 else []))
        _BUILT[sc.name] = dict(
            pack_d=d, cl=cl, pack=abi.make_pack(d), stars=abi.make_stars(cl), truth=truth, start=start,
            priors=synth.default_priors(d, truth, sc.n_pops), options=abi.make_options(sc.mode, sc.n_pops, sc.K or 8, sc.Q or 8),
            free=np.array(free, dtype=np.int32), chol=chol, ids=np.arange(WALKERS, dtype=np.int32),
            axes=[("age", abi.P_LOGAGE, [float(v) for v in la])] + ([("feh", abi.P_FEH, [float(v) for v in fe])] if long_feh else []))
    return _BUILT[sc.name]


def run_twin(sc, b, evaluate, lp0, ids=None):
    ids = b["ids"] if ids is None else np.asarray(ids, dtype=np.int32)
    return mcmc.HostBlockRunner(evaluate).run(b["start"][ids], np.asarray(lp0)[ids], ids, b["free"], b["chol"], sc.seed, 0, STEPS)


def crossings(sc, b, samples):
    """{(axis, boundary, direction, outcome): count} of a chain's proposals (ragged_walk.proposals restates them from the record)"""
    import ragged_walk as rw
    cur, prop = rw.proposals(b["start"], samples, list(b["free"]), b["chol"], sc.seed, 0, b["ids"])
    out = collections.Counter()
    free = list(b["free"])
    for name, col, ax in b["axes"]:
        for s in range(prop.shape[0]):
            for w in range(prop.shape[1]):
                took = np.array_equal(samples[s, w], prop[s, w][free]) and not np.array_equal(prop[s, w][free], cur[s, w][free])
                i0, x1 = bracket(ax, cur[s, w, col]), prop[s, w, col]
                i1 = bracket(ax, x1) if x1 <= ax[-1] else len(ax) - 1
                for label, t in thresholds(len(ax)).items():
                    if (i0 >= t) != (i1 >= t):
                        out[name, label, "up" if i1 > i0 else "down", "accepted" if took else "rejected"] += 1
    return out


def required_crossings(b):
    return [(name, label, dr, oc) for name, _, ax in b["axes"] for label in thresholds(len(ax)) for dr in ("up", "down")
            for oc in ("accepted", "rejected")]


# ---- R4: the WD branch on long tip columns -------------------------------------------------------------------------------------------
WD_PACKS = ("w17x129", "w3x3x513", "w513")
TIPS_LDS_MAX = 2048                                 # b9_device.h: B9_TIPS_LDS_MAX


def search_path(na, target):
    """The descending 8-ary search of a column of na tips (b9_star.hip.h: bracket8<true> / prec_corners) on its way to the
    answer `target` (the largest i with tips[i] >= m): ([the probed indices of every round], the start of the tail)."""
    lo, ln, rounds = 0, na - 1, []
    while ln >= 8:
        step = ln >> 3
        rounds.append([lo + j * step for j in range(1, 8)])
        c = min(7, (target - lo) // step)
        lo += c * step
        ln = ln - 7 * step if c == 7 else step
    return rounds, lo


def search_depth(na):
    return len(search_path(na, 0)[0])


def equal_tips_site(na):
    """the age index of the first of the two equal consecutive tips: the third probe of the search's first round"""
    return 3 * ((na - 1) >> 3)


@functools.lru_cache(maxsize=None)
def wd_pack(name):
    """(pack, rows): the pack with two equal consecutive tips on a probe position of column (FeH 0, Y 0) and one row in the LAST
    age cell -- every tip of every corner column lies above the derived tip, a mass can be light at one corner only --, FeH
    cell 0 and, where Y is an axis, population A in Y cell 0 and population B in Y cell 1."""
    d = dict(pack(name))
    d["mass"] = d["mass"].copy()
    na = len(d["log_age"])
    last = (d["iso_offset"] + d["iso_n_eep"] - 1)[:na]
    j = equal_tips_site(na)
    d["mass"][last[j + 1]] = d["mass"][last[j]]
    rows = [S._row(d, na - 2, 0.875, 0, 0.5, 0, 0.25)]
    return d, rows


def wd_packs():
    """tests/wd_seams.py's packs() for these packs: name -> (pack, rows)"""
    return {name: wd_pack(name) for name in WD_PACKS}


@functools.lru_cache(maxsize=None)
def _wd_cases(name):
    d, rows = wd_pack(name)
    row, up, na = rows[0], float(d["m_wd_up"]), len(d["log_age"])
    md = R.Model(R.REF, d, row)
    tip = float(md.tip.v)
    cols = list(md.tips.values())
    masses = []                                                    # (mass, wd_type)
    probes = set()
    for target in (equal_tips_site(na) + 1, na - 2):
        rounds, tail = search_path(na, target)
        probes |= {p for r in rounds for p in r} | {tail}
    probes |= {na - 2, na - 1}
    for c, t in enumerate(cols):
        for j in sorted(probes):
            masses += [(t[j], j & 1)] + ([(S._dn(t[j]), 0), (S._up(t[j]), 1)] if c < 2 else [])
            if c == 0 and j + 1 < na:
                masses.append((t[j + 1], 0))
            if c == 0 and j >= 1:
                masses.append((t[j - 1], 1))
        masses += [(0.5 * (tip + t[-1]), 0), (S._up(t[-1]), 1)]    # light at this corner (and not at one with smaller tips)
    t0s = sorted(t[0] for t in cols)
    masses += [(0.5 * (t0s[0] + t0s[-1]), 0), (0.5 * (t0s[-1] + up), 1)]     # heavy at one corner only; at every corner
    out, dropped = [], 0
    for m, ty in masses:
        if not tip < m <= up:
            continue
        c = dict(fam="b", pack=name, row=0, pop=0, m1=float(m), q=0.0, wd_type=int(ty))
        c["ref"] = R.evaluate(d, row, 0, c["m1"], 0.0, c["wd_type"], model=md)
        if S.meets_budget(c["ref"]) and not any(a == "nan" for a in c["ref"]["app_mags"]):
            out.append(c)
        else:
            dropped += 1                                           # (wd_seams' rule: a case whose decision rounding could turn is no case)
    assert len(out) <= 400 and dropped <= len(out) // 8, (len(out), dropped)
    return out


def wd_cases():
    """tests/wd_seams.py's cases() for these packs"""
    return [c for name in WD_PACKS for c in _wd_cases(name)]


# ---- R5: a saved chain hopping between the cells beside the boundaries -----------------------------------------------------------------
CHAIN_PACK, CHAIN_K, CHAIN_Q, CHAIN_WD_NODES = "a193", 1, 2, 63
CHAIN_CELLS = (0, 63, 64, 127, 128, 191)
CHAIN_TOKENS = (64, 63, 0, 128, 127, 191, 63, 64, 127, 128, 191, 0)
ChainSetting = collections.namedtuple("ChainSetting", "name n_filt n_pops")


def _chain_row(d, cell, frac):
    row = S._row(d, cell, frac, 0, 0.5)
    row[abi.P_MOD], row[abi.P_ABS], row[abi.P_CARBONICITY] = 10.2, 0.02, 0.38
    return row


@functools.lru_cache(maxsize=None)
def chain_problem():
    """tests/ragged_chain.py's problem() on the 193-age pack: a catalogue of 20 stars (3 of them WD-stage) drawn in each of the
    cells the script visits, and ONE script of 12 rows hopping between them."""
    import ragged_walk as rw
    import test_gpu_moments as tm
    import wdmoments_ref as wr
    d = pack(CHAIN_PACK)
    parts = [rw.catalogue(d, _chain_row(d, c, 0.4375), 20, 31 + 10 * k, wd_frac=3 / 20, n_pops=1) for k, c in enumerate(CHAIN_CELLS)]
    cl = dict(n_filt=d["n_filt"], truth=parts[0]["truth"])
    for key in tm.PER_STAR:
        cl[key] = np.ascontiguousarray(np.concatenate([np.asarray(p[key]) for p in parts]))
    cl["filter_prior_min"] = np.min([p["filter_prior_min"] for p in parts], axis=0)
    cl["filter_prior_max"] = np.max([p["filter_prior_max"] for p in parts], axis=0)
    rows = np.stack([_chain_row(d, c, (0.375, 0.625, 0.5)[i % 3]) for i, c in enumerate(CHAIN_TOKENS)])
    rows.setflags(write=False)
    return dict(setting=ChainSetting("long", d["n_filt"], 1), pack_d=d, cl=cl, n_pops=1, scripts=[rows], truth=cl["truth"],
                wd=wr.wd_stars(cl), n_stars=len(cl["mass1"]))


@functools.lru_cache(maxsize=None)
def chain_reference():
    """ragged_chain.Reference over chain_problem() (its constructor takes a setting's name; everything else is inherited)"""
    import ragged_chain as rcn
    import test_gpu_moments as tm

    class LongReference(rcn.Reference):
        def __init__(self, prob, K, Q):
            self.prob, self.K, self.Q = prob, K, Q
            self.n_nodes = tm.n_nodes_of(prob["pack_d"], prob["n_pops"], K, Q)
            self._memo = {}
            self.distinct = np.array(prob["scripts"][0])

    return LongReference(chain_problem(), CHAIN_K, CHAIN_Q)


# ---- R6: the heavy role's LDS ----------------------------------------------------------------------------------------------------------
LDS_PER_CU = 160 * 1024                             # b9_launch.h: B9_LDS_PER_CU


def heavy_lds_doubles(d, n_pops, n_cand, mass_cap):
    """b9_kernels.hip's heavy_lds_doubles for a pack dict with rectangular cooling tracks: 8 words of scratch, the packed axes
    (age axis, one cooling-age axis, WD mass, carbonicity, log Teff, log g axes, one word per track), the AGB tips -- the whole
    table up to B9_TIPS_LDS_MAX entries, else 4 corner columns per candidate and population --, the mass columns, the candidates'
    parameter rows, 8 words of over-read."""
    n_age, n_tips = len(d["log_age"]), len(d["iso_n_eep"])
    assert "wc_n_age" not in d
    n_tracks = max(1, len(d["wc_carb"])) * len(d["wc_mass"])
    hc = n_age + len(d["wc_log_age"]) + len(d["wc_mass"]) + max(1, len(d["wc_carb"])) + len(d["at_log_teff"]) + len(d["at_logg"]) + n_tracks
    tips = n_tips if n_tips <= TIPS_LDS_MAX else 4 * n_pops * n_cand * n_age
    return 8 + hc + tips + n_pops * n_cand * mass_cap + n_cand * abi.B9_NPARAM + 8


def capacity_pack(n_age):
    return grid_pack(3, 2, 1, n_age, 8)


def fused_step_lds_bytes(n_age, n_pops=2, n_cand=2):
    """dynamic LDS of the fused step (two candidates; n_cand = 1: of k_star_like and the tree launch) on capacity_pack(n_age):
    mass_cap = the longest isochrone, rounded to even"""
    d = capacity_pack(n_age)
    return 8 * heavy_lds_doubles(d, n_pops, n_cand, (int(d["iso_n_eep"].max()) + 1) & ~1)


def smallest_refused(n_cand):
    """the smallest age axis of capacity_pack whose two-population launch asks for more dynamic LDS than a compute unit has"""
    n = 2
    while fused_step_lds_bytes(n, 2, n_cand) <= LDS_PER_CU:
        n += max(1, (LDS_PER_CU - fused_step_lds_bytes(n, 2, n_cand)) // (2 * 8 * (8 * n_cand + 1)))
    assert fused_step_lds_bytes(n - 1, 2, n_cand) <= LDS_PER_CU < fused_step_lds_bytes(n, 2, n_cand)
    return n
