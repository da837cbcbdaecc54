"""Sampler blocks that walk across grid cells whose isochrones differ in length: the packs, the catalogues, numpy
restatements of what the fused marginalised step decides from a parameter row, the scripted cases and the chain comparator
shared by tests/test_ragged_walk_host.py (CPU) and tests/test_gpu_ragged_walk.py (GPU).  Pure numpy: nothing here needs a GPU.

The LADDER pack is smooth (synth._iso_points) on a fine grid -- 12 ages x 4 [Fe/H] x 1 or 3 Y, the axis spacing of the order
of a proposal step -- and every isochrone has its own first EEP and length, chosen so that the common EEP range of a cell
depends on its age index (LADDER_COMMON): the full length, 66 / 65 / 64 and 34 / 33 / 32 points ((n - 1) K just above, on
and just below a multiple of 64 for K = 1, 2 and, at 66 / 65 / 64, K = 3), 3 points, 2 points (one interval) and 1 point (no
isochrone).  A block of a few dozen steps whose walkers start in different cells therefore sees its node table grow, shrink,
vanish and come back."""
import collections

import numpy as np

from base_amd import abi, mcmc, synth

N_EEP_REF = 160                                     # the longest isochrone: 5 node chunks at K = 2
AGES = 9.60 + 0.012 * np.arange(12)
FEHS = -0.30 + 0.05 * np.arange(4)
YS = 0.25 + 0.012 * np.arange(3)
#: last EEP + 1 and lowest first EEP of the isochrones at every age point.  An isochrone's first EEP is FIRSTS[a] + 2 ((i_feh +
#: i_y + i_age) % 2): both age sides of a cell carry both offsets, so the cell's common range is [max(FIRSTS[a], FIRSTS[a + 1])
#: + 2, min(ENDS[a], ENDS[a + 1])).  The rungs 66 / 65 / 64 and 34 / 33 / 32 differ at the LOW end: the catalogues hold no star
#: below 0.15 solar masses (EEP 13), so a move between them costs next to nothing and is accepted as often as any other.  The
#: first trio shrinks towards younger ages, the second towards older ones (given-mass chains drift to younger ages: a star
#: heavier than the isochrone's tip is impossible).  The rungs of 3, 2 and 1 points lie below every star: the likelihood
#: there is the field's, and flat.
ENDS = np.array([70, 70, 70, 160, 160, 160, 40, 40, 40, 11, 11, 12])
FIRSTS = np.array([4, 3, 2, 0, 0, 0, 4, 5, 6, 6, 7, 8])
#: common EEPs of the cells of age index 0 .. 10
LADDER_COMMON = [64, 65, 66, 158, 158, 34, 33, 32, 3, 2, 1]
TRUTH_CELL = 3
FLAT_EEPS = (20, 21)                                # variant "flat": these two EEPs carry the same mass in every isochrone
SEC_ROWS = 24                                       # b9_marg_step.hip.h: B9_MSTEP_SEC_ROWS
VARIANTS = ("base", "flat", "wdragged")


def ladder_pack(n_filt, n_y=1, seed=0, variant="base", min_end=0):
    """The ladder pack as a dict of arrays (synth.make_pack's keys).  seed: shifts the grid by a fraction of a cell (the
    isochrones stay the analytic ones).  variant: "flat" = EEPs FLAT_EEPS of every isochrone share one mass (a node whose
    mass step is not positive), "wdragged" = every WD cooling track has its own age axis.  min_end: every isochrone reaches at
    least this EEP (the same pack padded at its upper end: tests/test_ragged_walk_host.py's stale_length)."""
    assert variant in VARIANTS and n_y in (1, 3)
    rng = np.random.default_rng(seed)
    log_age = AGES + 0.003 * rng.uniform(-1, 1)
    feh = FEHS + 0.01 * rng.uniform(-1, 1)
    y = YS.copy() if n_y == 3 else np.array([0.262])
    n_iso = len(feh) * len(y) * len(log_age)
    first, count, offset = np.zeros(n_iso, np.int32), np.zeros(n_iso, np.int32), np.zeros(n_iso, np.int64)
    masses, mags, off, k = [], [], 0, 0
    for i_f, fe in enumerate(feh):
        for i_y, yy in enumerate(y):
            for i_a, la in enumerate(log_age):
                f0 = int(FIRSTS[i_a]) + 2 * ((i_f + i_y + i_a) % 2)
                n = max(int(ENDS[i_a]), min(int(min_end), N_EEP_REF)) - f0
                ids = np.arange(f0, f0 + n, dtype=np.float64)
                m, mg = synth._iso_points(la, fe, yy, ids, N_EEP_REF, n_filt)
                if variant == "flat":
                    sel = np.flatnonzero(ids == FLAT_EEPS[1])
                    if sel.size:
                        m[sel[0]] = m[sel[0] - 1]
                first[k], count[k], offset[k] = f0, n, off
                masses.append(m); mags.append(mg)
                off += n; k += 1
    assert count.max() <= N_EEP_REF and count.min() >= 2          # (b9_load_pack takes no isochrone of one point)
    d = dict(name="ladder", n_filt=n_filt, feh=feh, y=y, log_age=log_age, iso_first_eep=first, iso_n_eep=count, iso_offset=offset,
             mass=np.concatenate(masses), mags=np.concatenate(mags, axis=0),
             abs_coeff=(synth.ABS_COEFF_8[:n_filt] if n_filt <= 8 else np.linspace(1.6, 0.1, n_filt)),
             filters=[f"F{i}" for i in range(n_filt)], ifmr_id=abi.IFMR_WILLIAMS, m_wd_up=8.0)
    d.update(synth.make_wd_tables(n_filt, ragged=variant == "wdragged"))
    for i_f in range(0 if min_end else len(feh) - 1):
        got = [common_range(d, _cell_row(d, a, i_f), 0)[1] for a in range(len(log_age) - 1)]
        assert got == LADDER_COMMON, got
    return d


def _cell_row(pack, i_age, i_feh, frac=0.5):
    """A parameter row inside cell (i_age, i_feh) (Y and Y2 in the first Y cell)."""
    la, fe, yy = pack["log_age"], pack["feh"], pack["y"]
    row = synth.default_params(pack, log_age=la[i_age] + frac * (la[i_age + 1] - la[i_age]),
                               feh=fe[i_feh] + frac * (fe[i_feh + 1] - fe[i_feh]), mod=10.2, av=0.02)
    if len(yy) > 1:
        row[abi.P_Y], row[abi.P_Y2] = yy[0] + 0.4 * (yy[1] - yy[0]), yy[1] + 0.6 * (yy[2] - yy[1])
    return row


def truth_row(pack):
    """The catalogues' truth: inside a long cell."""
    return _cell_row(pack, TRUTH_CELL, 1, 0.45)


def catalogue(pack, truth, n_stars, seed, wd_frac=0.08, n_pops=1, sigma_scale=3.0):
    """synth.make_cluster at `truth`, its errors widened by sigma_scale (so that moves between cells are accepted at all)."""
    assert n_stars <= 200
    cl = synth.make_cluster(pack, n_stars, seed=seed, truth=truth, wd_frac=wd_frac, n_pops=n_pops, field_frac=0.03, unused_frac=0.02)
    rng = np.random.default_rng(seed + 1)
    sg = np.asarray(cl["sigma"], dtype=np.float64)
    used = sg > 0
    extra = np.sqrt(sigma_scale ** 2 - 1.0) * np.where(used, sg, 0.0)
    cl["obs"] = cl["obs"] + rng.normal(size=sg.shape) * extra
    cl["sigma"] = np.where(used, sg * sigma_scale, sg)
    cl["filter_prior_min"] = np.minimum(cl["filter_prior_min"], cl["obs"].min(axis=0) - 0.5)
    cl["filter_prior_max"] = np.maximum(cl["filter_prior_max"], cl["obs"].max(axis=0) + 0.5)
    return cl


def field_terms(cl):
    """log(1 - p) + log fs of every star: what its value is when the cluster explains nothing of it."""
    log_fs = -np.log(np.asarray(cl["filter_prior_max"]) - np.asarray(cl["filter_prior_min"])).sum()
    return np.log1p(-np.asarray(cl["clust_prior"])) + log_fs


def dominance(perstar, cl):
    """fraction of the stars whose value exceeds their field term by more than log 2: the cluster term is the larger one"""
    return float(np.mean(perstar - field_terms(cl) > np.log(2.0)))


# ---- restatements: what a parameter row makes of the pack ------------------------------------------------------------------
def _bracket(ax, x):
    return int(np.clip(np.searchsorted(ax, x, side="right") - 1, 0, len(ax) - 2))


def cell_of(pack, row, pop=0):
    """((i_age, i_feh, i_y), names of the axes the row lies outside of)"""
    la, fe, yy = pack["log_age"], pack["feh"], pack["y"]
    y = row[abi.P_Y2 if pop else abi.P_Y]
    out = []
    if not la[0] <= row[abi.P_LOGAGE] <= la[-1]: out.append("age")
    if not fe[0] <= row[abi.P_FEH] <= fe[-1]: out.append("feh")
    if len(yy) > 1 and not yy[0] <= y <= yy[-1]: out.append("y")
    return (_bracket(la, row[abi.P_LOGAGE]), _bracket(fe, row[abi.P_FEH]), _bracket(yy, y) if len(yy) > 1 else 0), out


def common_range(pack, row, pop=0):
    """(valid, n, first): the common EEP range of the corner isochrones of the row's cell (header_of: valid = inside the grid
    and at least two common points)."""
    (ia, i_f, iy), out = cell_of(pack, row, pop)
    nA, nY = len(pack["log_age"]), len(pack["y"])
    lo, hi = -10 ** 9, 10 ** 9
    for df in range(2):
        for dy in range(2 if nY > 1 else 1):
            for da in range(2):
                k = ((i_f + df) * nY + iy + dy) * nA + ia + da
                lo = max(lo, int(pack["iso_first_eep"][k]))
                hi = min(hi, int(pack["iso_first_eep"][k]) + int(pack["iso_n_eep"][k]))
    n = hi - lo
    return (not out) and n >= 2, n, lo


def n_chunks(pack, row, K, pop=0):
    """64-node chunks of the row's node table ((n - 1) K nodes); 0 where there is no isochrone"""
    valid, n, _ = common_range(pack, row, pop)
    return ((n - 1) * K + 63) // 64 if valid else 0


def mass_column(pack, row, pop=0):
    iso = synth.derive_isochrone(pack, row[abi.P_LOGAGE], row[abi.P_FEH], row[abi.P_Y2 if pop else abi.P_Y])
    return None if iso is None else iso[1]


def companion_runs(mass, K, Q):
    """{(chunk, j): lmax - lmin + 2} over the chunk's nodes that exist, have a positive mass step and whose companion of mass
    (j / Q) m1 is not below the isochrone's first point -- the row count marg_build_table compares with SEC_ROWS; 0 where no
    node of the chunk has such a companion."""
    n = len(mass)
    n_nodes = (n - 1) * K
    node = np.arange(((n_nodes + 63) // 64) * 64)
    live = node < n_nodes
    e = np.where(live, node // K, 0)
    s = node - e * K
    a, d = mass[e], mass[e + 1] - mass[e]
    ok = live & (d > 0)
    m1 = s * (d / K) + a
    runs = {}
    for j in range(1, Q):
        m2 = (j / Q) * m1
        lo2 = np.clip(np.searchsorted(mass[:n - 1], m2, side="right") - 1, 0, n - 2)
        need = ok & ~(m2 < mass[0])
        for c in range(len(node) // 64):
            sel = need[c * 64:(c + 1) * 64]
            l = lo2[c * 64:(c + 1) * 64][sel]
            runs[(c, j)] = int(l.max() - l.min() + 2) if l.size else 0
    return runs


# ---- the tagger --------------------------------------------------------------------------------------------------------------
TAGS = (["cell_changed:" + a for a in ("age", "feh", "y")] + ["chunks_grew", "chunks_shrank", "one_interval", "flat_segment"]
        + ["invalid:grid:" + a for a in ("age", "feh", "y")] + ["invalid:eeps", "invalid:prior", "valid_after_invalid"]
        + ["run_le_24", "run_eq_24", "run_eq_25", "run_gt_24"])


def proposals(start, samples, free, chol, seed, step0, ids):
    """(cur[T, W, 12], prop[T, W, 12]): every step's state before it and its proposal, HostBlockRunner's arithmetic"""
    T, W, d = samples.shape
    cur, prop = np.empty((T, W, abi.B9_NPARAM)), np.empty((T, W, abi.B9_NPARAM))
    state = np.array(start, dtype=np.float64)
    for s in range(T):
        z, _ = mcmc.draws(seed, step0 + s, ids, d)
        delta = np.zeros_like(z)
        for j in range(d):
            delta = delta + chol[None, :, j] * z[:, j:j + 1]
        cur[s] = state
        prop[s] = state
        prop[s][:, free] += delta
        state = state.copy()
        state[:, free] = samples[s]
    return cur, prop


class _RowFacts:
    """what the tagger needs of a row, per population, computed once per distinct row"""

    def __init__(self, pack, n_pops, K, Q):
        self.pack, self.n_pops, self.K, self.Q, self.memo = pack, n_pops, K, Q, {}

    def __call__(self, row):
        key = row.tobytes()
        if key not in self.memo:
            self.memo[key] = self._facts(row)
        return self.memo[key]

    def _facts(self, row):
        pack, f = self.pack, dict(bad=[], cells=[], chunks=[], n=[], flat=False, runs=[])
        if row[abi.P_ABS] < 0.0 or (self.n_pops == 2 and not 0.0 <= row[abi.P_LAMBDA] <= 1.0):
            f["bad"].append("invalid:prior")
        for pop in range(self.n_pops):
            cell, out = cell_of(pack, row, pop)
            valid, n, _ = common_range(pack, row, pop)
            f["bad"] += ["invalid:grid:" + a for a in out]
            if not out and not valid:
                f["bad"].append("invalid:eeps")
            f["cells"].append(cell)
            f["n"].append(n if valid else 0)
            f["chunks"].append(((n - 1) * self.K + 63) // 64 if valid else 0)
        if not f["bad"]:
            for pop in range(self.n_pops):
                mass = mass_column(pack, row, pop)
                f["flat"] = f["flat"] or bool(np.any(np.diff(mass) <= 0))
                if self.Q:
                    f["runs"] += [r for r in companion_runs(mass, self.K, self.Q).values() if r > 0]
        return f


def walk_tags(block):
    """The tags a block reached.  block: dict(pack, n_pops, K, Q (0, 0 = given-mass mode: no node table and no companion runs; its
    `chunks` are those the row's table would have at K = 2), start, samples, free, chol, seed, step0,
    ids).  Returns dict(proposed, accepted: Counter of TAGS; chunks: (fewest, most) node chunks among the valid rows met;
    runs: the companion-run lengths met; n_steps, n_invalid, n_accept; shorter: the steps at which a walker moved to a row
    of fewer common EEPs)."""
    pack, n_pops = block["pack"], block["n_pops"]
    facts = _RowFacts(pack, n_pops, block["K"] or 2, block["Q"])
    cur, prop = proposals(block["start"], block["samples"], block["free"], block["chol"], block["seed"], block["step0"], block["ids"])
    T, W, _ = prop.shape
    free = list(block["free"])
    proposed, accepted = collections.Counter(), collections.Counter()
    chunks, runs, n_invalid, n_accept, shorter = set(), set(), 0, 0, []
    last_invalid = [False] * W
    for s in range(T):
        for w in range(W):
            p, c = facts(prop[s, w]), facts(cur[s, w])
            took = np.array_equal(block["samples"][s, w], prop[s, w][free]) and not np.array_equal(prop[s, w][free], cur[s, w][free])
            tags = set(p["bad"])
            if p["bad"]:
                n_invalid += 1
                assert not took
            else:
                for k in range(n_pops):
                    for i, a in enumerate(("age", "feh", "y")):
                        if p["cells"][k][i] != c["cells"][k][i]:
                            tags.add("cell_changed:" + a)
                    if p["chunks"][k] > c["chunks"][k]: tags.add("chunks_grew")
                    if p["chunks"][k] < c["chunks"][k]: tags.add("chunks_shrank")
                    if p["n"][k] == 2: tags.add("one_interval")
                if p["flat"]: tags.add("flat_segment")
                if last_invalid[w]: tags.add("valid_after_invalid")
                r = p["runs"]
                if any(x <= SEC_ROWS for x in r): tags.add("run_le_24")
                if any(x == SEC_ROWS for x in r): tags.add("run_eq_24")
                if any(x == SEC_ROWS + 1 for x in r): tags.add("run_eq_25")
                if any(x > SEC_ROWS for x in r): tags.add("run_gt_24")
                chunks.update(p["chunks"])
                runs.update(r)
            last_invalid[w] = bool(p["bad"])
            proposed.update(tags)
            if took:
                accepted.update(tags)
                n_accept += 1
                if any(p["n"][k] < c["n"][k] for k in range(n_pops)):
                    shorter.append(s)
    return dict(proposed=proposed, accepted=accepted, chunks=(min(chunks), max(chunks)) if chunks else (0, 0), runs=sorted(runs),
                n_steps=T * W, n_invalid=n_invalid, n_accept=n_accept, shorter=shorter)


# ---- the scripted cases ------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name variant n_filt n_pops mode K Q seed walkers steps scale cells")
GIVEN, MARG = abi.MODE_GIVEN_MASS, abi.MODE_MARGINALISED
N_STARS = 100


def free_of(n_pops):
    return np.array(list(mcmc.DEFAULT_FREE) + ([abi.P_Y, abi.P_Y2, abi.P_LAMBDA] if n_pops == 2 else []))


def chol_of(n_pops, scale):
    return np.diag([3e-3, 1.2e-2, 8e-3, 6e-3] + ([2e-3, 2e-3, 4e-2] if n_pops == 2 else [])) * scale


#: name, pack variant, filters, populations, mode, K, Q, seed, walkers, steps, step scale, age index of every walker's first cell.
#: Seeds and scales were chosen on the CPU (tests/test_ragged_walk_host.py states what they had to satisfy).
CASES = [
    Case("m-3f-1p-k2q2", "base", 3, 1, MARG, 2, 2, 1, 5, 30, 3.0, (3, 2, 1, 6, 9)),
    Case("m-8f-2p-k1q2", "base", 8, 2, MARG, 1, 2, 21, 5, 30, 3.0, (2, 1, 5, 8, 9)),
    Case("m-12f-1p-k1q2-flat", "flat", 12, 1, MARG, 1, 2, 5, 5, 30, 3.0, (4, 2, 1, 6, 9)),
    Case("m-8f-1p-k3q2-wdragged", "wdragged", 8, 1, MARG, 3, 2, 6, 5, 30, 3.0, (2, 0, 5, 8, 9)),
    Case("m-12f-2p-k2q2", "base", 12, 2, MARG, 2, 2, 7, 5, 30, 3.0, (2, 1, 5, 6, 9)),
    Case("m-3f-2p-k2q4-flat", "flat", 3, 2, MARG, 2, 4, 8, 4, 24, 3.0, (1, 5, 6, 9)),
    Case("g-3f-1p", "base", 3, 1, GIVEN, 0, 0, 21, 5, 40, 3.0, (3, 2, 1, 6, 9)),
    Case("g-8f-2p", "base", 8, 2, GIVEN, 0, 0, 4, 5, 40, 3.0, (2, 1, 5, 8, 9)),
    Case("g-12f-1p-flat", "flat", 12, 1, GIVEN, 0, 0, 9, 5, 40, 3.0, (2, 2, 5, 6, 9)),
    Case("g-8f-1p-wdragged", "wdragged", 8, 1, GIVEN, 0, 0, 21, 5, 40, 3.0, (4, 2, 5, 6, 8)),
    Case("g-12f-2p-flat", "flat", 12, 2, GIVEN, 0, 0, 11, 5, 40, 3.0, (2, 1, 5, 6, 9)),
    Case("g-3f-2p", "base", 3, 2, GIVEN, 0, 0, 22, 5, 40, 3.0, (2, 2, 5, 6, 9)),
]
MARG_CASES = [c for c in CASES if c.mode == MARG]
GIVEN_CASES = [c for c in CASES if c.mode == GIVEN]

_BUILT = {}


def build_case(case):
    """dict(pack_d, cl, pack, stars, priors, options, truth, start, free, chol, ids) of a case; built once per process and left
    unchanged.  A walker starts in the cell of age index case.cells[w], a little off its middle."""
    if case.name not in _BUILT:
        pack_d = ladder_pack(case.n_filt, 3 if case.n_pops == 2 else 1, case.seed, case.variant)
        truth = truth_row(pack_d)
        cl = catalogue(pack_d, truth, N_STARS, case.seed, 0.08, case.n_pops)
        rng = np.random.default_rng(case.seed + 7)
        start = np.tile(truth, (case.walkers, 1))
        la = pack_d["log_age"]
        for w, a in enumerate(case.cells):
            start[w, abi.P_LOGAGE] = la[a] + rng.uniform(0.3, 0.7) * (la[a + 1] - la[a])
            start[w, abi.P_FEH] += rng.uniform(-0.02, 0.02)
            start[w, abi.P_MOD] += rng.normal(0, 0.01)
        _BUILT[case.name] = dict(
            pack_d=pack_d, cl=cl, pack=abi.make_pack(pack_d), stars=abi.make_stars(cl), truth=truth, start=start,
            priors=synth.default_priors(pack_d, truth, case.n_pops), options=abi.make_options(case.mode, case.n_pops, case.K or 8, case.Q or 8),
            free=free_of(case.n_pops), chol=chol_of(case.n_pops, case.scale), ids=np.arange(case.walkers))
    return _BUILT[case.name]


def block_of(case, b, samples):
    return dict(pack=b["pack_d"], n_pops=case.n_pops, K=case.K, Q=case.Q, start=b["start"], samples=samples, free=b["free"],
                chol=b["chol"], seed=case.seed, step0=0, ids=b["ids"])


# ---- the comparator ----------------------------------------------------------------------------------------------------------
class ChainMismatch(AssertionError):
    def __init__(self, step, what, detail=""):
        super().__init__(f"step {step}: {what} {detail}")
        self.step, self.what = step, what


def compare_chains(got, want, lp_rtol=1e-10):
    """A block's (params, logpost, samples, lps, n_accept) against the host twin's: positions to rtol 1e-12 / atol 1e-13, the
    same log-posteriors finite and those equal to lp_rtol, no NaN, equal accept counts.  Raises ChainMismatch naming the first
    step that differs."""
    gs, gl, ws, wl = got[2], got[3], want[2], want[3]
    assert gs.shape == ws.shape and gl.shape == wl.shape
    for s in range(ws.shape[0]):
        if np.isnan(gs[s]).any() or np.isnan(gl[s]).any():
            raise ChainMismatch(s, "nan")
        if not np.allclose(gs[s], ws[s], rtol=1e-12, atol=1e-13):
            raise ChainMismatch(s, "position", f"{gs[s]} != {ws[s]}")
        fin = np.isfinite(wl[s])
        if not np.array_equal(np.isfinite(gl[s]), fin):
            raise ChainMismatch(s, "finite", f"{gl[s]} != {wl[s]}")
        if not np.allclose(gl[s][fin], wl[s][fin], rtol=lp_rtol, atol=0):
            raise ChainMismatch(s, "logpost", f"{gl[s]} != {wl[s]}")
    T = ws.shape[0]
    if got[4] != want[4]:
        raise ChainMismatch(T, "accepts", f"{got[4]} != {want[4]}")
    # the state the block hands back
    if np.isnan(got[0]).any() or np.isnan(got[1]).any():
        raise ChainMismatch(T, "nan")
    if not np.allclose(got[0], want[0], rtol=1e-12, atol=1e-13):
        raise ChainMismatch(T, "final position")
    if not np.array_equal(np.isfinite(got[1]), np.isfinite(want[1])) or not np.allclose(got[1], want[1], rtol=lp_rtol, atol=0):
        raise ChainMismatch(T, "final logpost", f"{got[1]} != {want[1]}")


# ---- the oracle-driven chain of a case, with every evaluation kept ---------------------------------------------------------------
class Logged:
    """an evaluator that keeps every call's rows and values"""

    def __init__(self, evaluate):
        self.evaluate, self.rows, self.vals = evaluate, [], []

    def __call__(self, rows):
        v = np.asarray(self.evaluate(rows), dtype=np.float64)
        self.rows.append(np.array(rows)); self.vals.append(v.copy())
        return v


def run_twin(case, b, evaluate, lp0):
    return mcmc.HostBlockRunner(evaluate).run(b["start"], lp0, b["ids"], b["free"], b["chol"], case.seed, 0, case.steps)


def decision_margins(case, b, lp0, chain, log):
    """|log u - (lp(proposal) - lp(state))| of every decision [steps, W] (inf where the proposal has no log-posterior)"""
    out = np.empty((case.steps, case.walkers))
    for s in range(case.steps):
        _, u = mcmc.draws(case.seed, s, b["ids"], len(b["free"]))
        cur = lp0 if s == 0 else chain[3][s - 1]
        with np.errstate(invalid="ignore"):
            out[s] = np.where(np.isfinite(log.vals[s]), np.abs(np.log(u) - (log.vals[s] - cur)), np.inf)
    return out
