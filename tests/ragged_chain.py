"""The reductions over a saved chain on rows whose isochrones differ in length: the pack settings, the rung catalogue, the
scripted row lists with their tagger, the references of the eight calls (each the family's own reference, fed the rows' nodes)
with the family's own comparators, and the faulty stand-ins, shared by tests/test_ragged_chain_host.py (CPU) and
tests/test_gpu_ragged_chain.py (GPU).  Pure numpy: nothing here needs a GPU.

The pack is tests/ragged_walk.py's ladder pack: the cells of one age index share 158, 66 / 65 / 64, 34 / 33 / 32, 3, 2 and 1
common EEPs.  A script is an ordered list of 35 to 38 parameter rows inside those cells (and outside the grid): consecutive rows
have node tables of (n - 1) K nodes that grow, shrink, vanish and come back, inside a chunk of 32 rows and across the seam
between rows 31 and 32.  No tolerance is stated here: every comparison goes through the check module of the call's family."""
import collections
import contextlib
import functools
import os
import re

import numpy as np

import masshist_check as hc
import masshist_ref as hr
import moments_ref as mr
import numpy_ref
import pointwise_check as pc
import pointwise_ref as pr
import ragged_walk as rw
import resid_check as rc
import resid_ref as rr
import starbins_check as sc
import starbins_ref as sr
import test_gpu_moments as tm
import wd_check
import wdbins_check as bc
import wdbins_ref as br
import wdmoments_check as wc
import wdmoments_ref as wr
from base_amd import abi, synth

CSRC = os.path.join(abi.REPO_ROOT, "base_amd", "csrc")

# ---- the settings ------------------------------------------------------------------------------------------------------------
Setting = collections.namedtuple("Setting", "name variant n_filt n_y n_pops")
SETTINGS = {s.name: s for s in (Setting("base4", "base", 4, 1, 1), Setting("wdragged5", "wdragged", 5, 3, 2),
                                Setting("base9", "base", 9, 1, 1))}
#: (setting, K, Q): every setting at K = 1, 2, 3 with Q = 2, and one case at Q = 4
COMBOS = [(s, K, 2) for s in SETTINGS for K in (1, 2, 3)] + [("base4", 2, 4)]
PACK_SEED, CAT_SEED = 0, 5
CHUNK = 32                                          # rows of a chunk of every call at these sizes (chunk_rows_of_the_calls)
LONGEST = 158
WD_NODES = (63, 65)                                 # n_nodes of the b9_wd_* calls
TAIL = 3                                            # b9_pointwise's tail length
HIST_BINS, STAR_BINS, WD_BINS = 33, 6, 4          # 33: two tiles of bins in b9_mass_hist

#: rung class -> the age cells that have it, the first being the cell its stars of the rung catalogue are drawn in
RUNGS = collections.OrderedDict([("158", (3, 4)), ("64-66", (1, 0, 2)), ("32-34", (6, 5, 7)), ("3", (8,)), ("2", (9,))])
INVALID_CELL = 10                                   # one common EEP: no isochrone
PER_RUNG, WD_PER_RUNG = 28, 5


# ---- the rung catalogue --------------------------------------------------------------------------------------------------------
def placed_catalogue(pack_d, truth, n_stars, n_wd, seed, n_pops, sigma=0.06):
    """A catalogue placed by hand in a cell whose isochrone ends below synth.make_cluster's lowest mass: MS-stage stars at masses
    inside the derived isochrone at three mass ratios, WD-stage stars above its tip whose precursor has died; the observations
    are the forward model's plus noise of `sigma` (of the order of the magnitude step between two nodes of these cells)."""
    rng = np.random.default_rng(seed)
    nf = pack_d["n_filt"]
    pop = (rng.random(n_stars) >= truth[abi.P_LAMBDA]).astype(np.int32) if n_pops == 2 else np.zeros(n_stars, np.int32)
    stage = np.full(n_stars, abi.STAGE_MSRG, np.int32)
    stage[np.arange(n_wd) * (n_stars // max(n_wd, 1)) + 1] = abi.STAGE_WD
    wd = stage == abi.STAGE_WD
    mass1 = np.empty(n_stars)
    for k in range(n_pops):
        iso = synth.derive_isochrone(pack_d, truth[abi.P_LOGAGE], truth[abi.P_FEH], truth[abi.P_Y2 if k else abi.P_Y])
        m0, tip = iso[1][0], iso[1][-1]
        sel = pop == k
        mass1[sel & ~wd] = m0 + (tip - m0) * rng.uniform(0.05, 0.95, int((sel & ~wd).sum()))
        # WD-stage stars whose precursor has died at `truth`: one that has not is observed at the forward model's marker
        # magnitude, fits only the nodes without a cooling age and leaves the derived sums of b9_wd_moments without a scale
        # ... and of at least one solar mass: above the band of masses in which this pack's column of AGB-tip masses, which is
        # not descending in age, gives the inversion for the precursor's age more than one answer (tip_inversion_ambiguous)
        cand = rng.uniform(1.0, pack_d["m_wd_up"] * 0.5, 256)
        cand = cand[wd_check.wd_chain(pack_d, truth, cand, pop=k)[1] < truth[abi.P_LOGAGE]]
        mass1[sel & wd] = cand[:int((sel & wd).sum())]
    q = np.array([0.0, 0.5, 0.97])[np.arange(n_stars) % 3]
    q[wd] = 0.0
    wd_type = (rng.random(n_stars) < 0.2).astype(np.int32)
    pred = synth.forward_mags(pack_d, truth, mass1, q, wd_type, pop=0)
    if n_pops == 2 and pop.any():
        pred[pop == 1] = synth.forward_mags(pack_d, truth, mass1[pop == 1], q[pop == 1], wd_type[pop == 1], pop=1)
    obs = pred + rng.normal(size=pred.shape) * sigma
    prior = np.clip(rng.normal(0.9, 0.05, n_stars), 0.5, 0.999)
    return dict(n_filt=nf, obs=obs, sigma=np.full(pred.shape, sigma), mass1=mass1, mass_ratio=q, clust_prior=prior, stage=stage,
                wd_type=wd_type, filter_prior_min=obs.min(axis=0) - 0.5, filter_prior_max=obs.max(axis=0) + 0.5, truth=truth,
                is_field=np.zeros(n_stars, bool), pop=pop)


def rung_catalogue(pack_d, n_pops, seed=CAT_SEED):
    """(cl, rung [star]: the index into RUNGS of the class the star was drawn in).  The concatenation of one small catalogue per
    rung class -- ragged_walk.catalogue (synth.make_cluster, errors widened) where the cell reaches make_cluster's lowest mass,
    placed_catalogue in the cells of 3 and 2 points -- with the filter-prior box that holds them all."""
    parts = []
    for k, (name, cells) in enumerate(RUNGS.items()):
        truth = rw._cell_row(pack_d, cells[0], 1, 0.45)
        if name in ("3", "2"):
            parts.append(placed_catalogue(pack_d, truth, PER_RUNG, WD_PER_RUNG, seed + 10 * k, n_pops))
        else:
            parts.append(rw.catalogue(pack_d, truth, PER_RUNG, seed + 10 * k, wd_frac=WD_PER_RUNG / PER_RUNG, n_pops=n_pops))
    cl = dict(n_filt=pack_d["n_filt"], truth=parts[0]["truth"])
    for key in tm.PER_STAR:
        cl[key] = np.ascontiguousarray(np.concatenate([np.asarray(p[key]) for p in parts]))
    cl["filter_prior_min"] = np.min([p["filter_prior_min"] for p in parts], axis=0)
    cl["filter_prior_max"] = np.max([p["filter_prior_max"] for p in parts], axis=0)
    assert len(cl["mass1"]) <= 200
    return cl, np.repeat(np.arange(len(RUNGS)), PER_RUNG)


# ---- the scripts ---------------------------------------------------------------------------------------------------------------
OUT = "O"                                           # a row outside the grid
#: rows 0 .. 23 of every script: every transition inside a chunk, for K = 1, 2 and 3
TOUR = [3, 9, 3, 2, 1, 2, INVALID_CELL, 4, OUT, 5, 6, 5, 7, 0, 3, 8, INVALID_CELL, 9, OUT, 9, 4, 1, 6, 3]
FILLER = [7, 0, 8, 6, 2, 5, 1]                      # rows 24 .. 30
#: rows 31 and 32 of script k: the transition that crosses the seam
SEAMS = [(3, 9), (9, 3), (1, 2), (2, 1), (INVALID_CELL, 4), (OUT, 5), (4, INVALID_CELL), (5, OUT), (3, 2), (2, 3)]
TAILS = [3, 6, 9, 0, 8]                             # rows 33 ..: 2 to 5 of them
VARIANTS = [(1, 0.35), (2, 0.6), (0, 0.5)]          # ([Fe/H] cell, frac) by (position + script) mod 3
N_SCRIPTS = len(SEAMS)


def script_tokens(k):
    f = FILLER[k % len(FILLER):] + FILLER[:k % len(FILLER)]
    return TOUR + f + list(SEAMS[k]) + TAILS[:2 + k % 4]


def token_row(pack_d, token, variant):
    i_feh, frac = VARIANTS[variant % len(VARIANTS)]
    if token == OUT:
        row = rw._cell_row(pack_d, 3, i_feh, frac)
        if variant % 2:
            row[abi.P_FEH] = pack_d["feh"][0] - 0.2
        else:
            row[abi.P_LOGAGE] = pack_d["log_age"][-1] + 1.0
        return row
    return rw._cell_row(pack_d, token, i_feh, frac)


def script_rows(pack_d, k):
    """rows [n, 12] of script k on this pack"""
    return np.stack([token_row(pack_d, t, pos + k) for pos, t in enumerate(script_tokens(k))])


TRANSITIONS = ("grew_one", "grew_several", "shrank_one", "shrank_several", "one_interval_after_longest", "longest_after_one_interval",
               "invalid_row", "outside_row", "valid_after_invalid", "valid_after_outside")
SIDES = ("inside", "across")


def row_facts(pack_d, row, K, n_pops):
    """(kind, n, chunks): kind "valid" / "invalid" (inside the grid, fewer than two common EEPs) / "outside"; n and chunks the
    largest over the populations (in the ladder pack they are one value: the cells of an age index share their common range)."""
    kinds, ns, cs = [], [], []
    for pop in range(n_pops):
        _, out = rw.cell_of(pack_d, row, pop)
        valid, n, _ = rw.common_range(pack_d, row, pop)
        kinds.append("outside" if out else ("valid" if valid else "invalid"))
        ns.append(n if valid else 0)
        cs.append(rw.n_chunks(pack_d, row, K, pop))
    kind = "outside" if "outside" in kinds else ("invalid" if "invalid" in kinds else "valid")
    return kind, max(ns), max(cs)


def script_tags(pack_d, rows, K, n_pops, chunk=CHUNK):
    """Counter of "<transition>@<side>" over the script's rows (side: `across` where row j opens a chunk, j > 0, else `inside`)
    and of "mod<r>" for (n - 1) K mod 64 = r of its valid rows, from the restatements of tests/ragged_walk.py alone."""
    facts = [row_facts(pack_d, r, K, n_pops) for r in rows]
    tags = collections.Counter()
    for j, (kind, n, c) in enumerate(facts):
        if kind == "valid":
            tags[f"mod{(n - 1) * K % 64}"] += 1
        if j == 0:
            continue
        side = "across" if j % chunk == 0 else "inside"
        pk, pn, pcn = facts[j - 1]
        here = []
        if kind == "invalid": here.append("invalid_row")
        if kind == "outside": here.append("outside_row")
        if kind == "valid" and pk == "invalid": here.append("valid_after_invalid")
        if kind == "valid" and pk == "outside": here.append("valid_after_outside")
        if kind == "valid" and pk == "valid":
            d = c - pcn
            if d == 1: here.append("grew_one")
            if d > 1: here.append("grew_several")
            if d == -1: here.append("shrank_one")
            if d < -1: here.append("shrank_several")
            if n == 2 and pn == LONGEST: here.append("one_interval_after_longest")
            if n == LONGEST and pn == 2: here.append("longest_after_one_interval")
        for t in here:
            tags[f"{t}@{side}"] += 1
    return tags


def _define(name, text):
    m = re.search(r"#define\s+" + name + r"\s+\(?\(?(?:size_t\)?)?\s*(\d+)\s*(?:<<\s*(\d+))?", text)
    assert m, name
    return int(m.group(1)) << int(m.group(2) or 0)


def chunk_rows_of_the_calls(n_stars, n_filt):
    """{call: rows of a chunk} of the five chain_reduce calls at this catalogue size, from the sources' row caps and scratch rule
    (mom_chunk_rows: as many rows as keep 8 n_stars n_col bytes a row within the call's scratch, at most the cap)."""
    ev = open(os.path.join(CSRC, "b9_capi_eval.cpp")).read()
    la = open(os.path.join(CSRC, "b9_launch.h")).read()
    ncol = {"MOM": abi.MOM_N, "HIST": HIST_BINS + 1, "SBIN": STAR_BINS + 3, "RESID": 2 + 2 * n_filt, "PW": 1}
    out = {}
    for key, nc in ncol.items():
        cap = _define(f"B9_{key}_MAX_ROWS", la if key == "PW" else ev)
        scratch = _define(f"B9_{key}_SCRATCH_BYTES", ev)
        out[key] = max(1, min(cap, scratch // max(1, 8 * n_stars * nc)))
    return out


def tip_inversion_ambiguous(pack_d, par, pop, m):
    """[node]: does the precursor's age of a WD progenitor of mass m have more than one answer at this row?  The WD branch inverts
    the column of AGB-tip masses over the age axis, corner by corner, taking it to descend with age (oracle/b9_oracle.c and
    base_amd/csrc/b9_star.hip.h :: prec_log_age_corner say so); the ladder pack's column does not -- its isochrones are cut at
    other EEPs from age to age -- so for a mass that the column passes more than once a bisection (the oracle's, numpy's) and the
    device's 8-ary search may stop at different crossings.  True where that can happen in one of the row's corners."""
    la, yy = pack_d["log_age"], pack_d["y"]
    nA, nY = len(la), len(yy)
    (_, i_f, iy), _ = rw.cell_of(pack_d, par, pop)
    tips_all = pack_d["mass"][pack_d["iso_offset"] + pack_d["iso_n_eep"] - 1]
    m = np.asarray(m, dtype=np.float64)
    out = np.zeros(len(m), dtype=bool)
    for df in range(2):
        for dy in range(2 if nY > 1 else 1):
            tips = tips_all[((i_f + df) * nY + iy + dy) * nA:][:nA]
            ge = tips[None, :] >= m[:, None]
            out |= ~np.all(ge[:, 1:] <= ge[:, :-1], axis=1) & (m <= tips[0]) & (m > tips[-1])
    return out


WD_FAMILY = ("sample_wd_mass", "wd_moments", "wd_bins")


def wd_family_chunk(call, n_rows, n_filt, n_pops, n_nodes, n_wd=0, n_bins=0, n_sel=6):
    """Rows of a chunk of b9_sample_wd_mass / b9_wd_moments / b9_wd_bins, from their drivers' own defines (b9_capi_eval.cpp): at
    most B9_WDS_MAX_ROWS, and as few as keep the chunk's node table -- n_pops n_nodes B9_WD?_NODE_DOUBLES(nfp) doubles a row --
    within B9_WDS_TABLE_BYTES (b9_wd_bins: and its per-(row, line) scratch within B9_WBIN_SCRATCH_BYTES).  These calls do NOT
    chunk at 32 rows and do not use the chain_reduce arena."""
    ev = open(os.path.join(CSRC, "b9_capi_eval.cpp")).read()
    ws = open(os.path.join(CSRC, "b9_wd_sample.hip.h")).read()
    nfp = 4 if n_filt <= 4 else (8 if n_filt <= 8 else 16)                 # b9_capi_stage.cpp: padded_filters
    node = 2 * nfp + 1 + _define("B9_WDS_DER", ws) + (0 if call == "sample_wd_mass" else 1)      # B9_WDS_ / B9_WDM_NODE_DOUBLES
    c = min(n_rows, _define("B9_WDS_MAX_ROWS", ev), _define("B9_WDS_TABLE_BYTES", ev) // (8 * n_pops * n_nodes * node))
    if call == "wd_bins":
        c = min(c, _define("B9_WBIN_SCRATCH_BYTES", ev) // (8 * n_wd * n_sel * (n_bins + 3)))
    return max(1, c)


def wd_seam_nodes(call, n_filt, n_pops, n_wd=0, n_bins=0):
    """the largest n_nodes at which the call's table rule gives chunks of CHUNK rows: the script's rows 31 | 32 then straddle a
    chunk boundary of the WD family too"""
    ev = open(os.path.join(CSRC, "b9_capi_eval.cpp")).read()
    ws = open(os.path.join(CSRC, "b9_wd_sample.hip.h")).read()
    nfp = 4 if n_filt <= 4 else (8 if n_filt <= 8 else 16)
    node = 2 * nfp + 1 + _define("B9_WDS_DER", ws) + (0 if call == "sample_wd_mass" else 1)
    n_nodes = _define("B9_WDS_TABLE_BYTES", ev) // (8 * n_pops * node * CHUNK)
    assert wd_family_chunk(call, 1000, n_filt, n_pops, n_nodes, n_wd, n_bins) == CHUNK
    return n_nodes


# ---- a problem: pack, catalogue, scripts, built once per setting ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problem(setting):
    s = SETTINGS[setting]
    pack_d = rw.ladder_pack(s.n_filt, s.n_y, PACK_SEED, s.variant)
    cl, rung = rung_catalogue(pack_d, s.n_pops)
    scripts = [script_rows(pack_d, k) for k in range(N_SCRIPTS)]
    for r in scripts:
        r.setflags(write=False)
    return dict(setting=s, pack_d=pack_d, cl=cl, rung=rung, n_pops=s.n_pops, scripts=scripts, truth=cl["truth"],
                wd=wr.wd_stars(cl), n_stars=len(cl["mass1"]))


def device_args(prob, K, Q):
    """(pack, stars, priors, options) for engine.Engine"""
    return (abi.make_pack(prob["pack_d"]), abi.make_stars(prob["cl"]), synth.default_priors(prob["pack_d"], prob["truth"], prob["n_pops"]),
            abi.make_options(mode=abi.MODE_GIVEN_MASS, n_pops=prob["n_pops"], marg_iso_increm=K, marg_n_q=Q))


# ---- the references: each family's own, fed the rows' nodes -------------------------------------------------------------------
def ms_nodes(prob, K, Q, rows):
    return [mr.star_nodes(prob["pack_d"], prob["cl"], par, prob["n_pops"], K, Q) for par in rows]


def wd_nodes(prob, n_nodes, rows):
    return [wr.star_nodes(prob["pack_d"], prob["cl"], par, prob["n_pops"], n_nodes) for par in rows]


def x_moments(prob, K, Q, rows, nodes):
    zero = np.zeros((prob["n_stars"], mr.N))
    return np.stack([zero if nodes[r] is None else mr.increments(prob["pack_d"], prob["cl"], par, prob["n_pops"], K, Q, nodes=nodes[r])
                     for r, par in enumerate(rows)])


def x_pointwise(prob, K, Q, rows, nodes):
    """(V [row, star] -- NaN in a row without nodes --, inside [row], live [row, star]): pointwise_ref.v_matrix's, from given nodes"""
    n = prob["n_stars"]
    V, inside, live = np.full((len(rows), n), np.nan), np.zeros(len(rows), bool), np.zeros((len(rows), n), bool)
    for r, par in enumerate(rows):
        if nodes[r] is not None:
            V[r], live[r] = pr.values(prob["pack_d"], prob["cl"], par, prob["n_pops"], K, Q, nodes=nodes[r])
            inside[r] = True
    return V, inside, live


def x_hist(prob, K, Q, rows, nodes, edges, quantity=hr.PRIMARY):
    zero = np.zeros((prob["n_stars"], len(edges)))
    return np.stack([zero if nodes[r] is None else hr.increments(prob["pack_d"], prob["cl"], par, prob["n_pops"], K, Q, quantity, edges, nodes=nodes[r])
                     for r, par in enumerate(rows)])


def x_bins(prob, K, Q, rows, nodes, edges, quantity=hr.PRIMARY):
    zero = np.zeros((prob["n_stars"], edges.shape[1] + 2))
    return np.stack([zero if nodes[r] is None else sr.increments(prob["pack_d"], prob["cl"], par, prob["n_pops"], K, Q, quantity, edges, nodes=nodes[r])
                     for r, par in enumerate(rows)])


def x_resid(prob, K, Q, rows, nodes):
    """(x, bound, absx), each [row, star, 2 + 2 nf]"""
    zero = np.zeros((prob["n_stars"], rr.ncol(prob["pack_d"]["n_filt"])))
    parts = [(zero, zero, zero) if nodes[r] is None else rr.increments(prob["pack_d"], prob["cl"], par, prob["n_pops"], K, Q, nodes=nodes[r])
             for r, par in enumerate(rows)]
    return tuple(np.stack([p[k] for p in parts]) for k in range(3))


def x_wd_moments(prob, n_nodes, rows, nodes):
    """(x [row, n_wd, 16], floor [row, n_wd, 16], amp [row, n_wd])"""
    n_wd = len(prob["wd"])
    none = (np.zeros((n_wd, wr.N)), np.zeros((n_wd, wr.N)), np.zeros(n_wd))
    ref = [none if nodes[r] is None else wr.increments(prob["pack_d"], prob["cl"], par, prob["n_pops"], n_nodes, want_extra=True, nodes=nodes[r])
           for r, par in enumerate(rows)]
    return tuple(np.stack([r[k] for r in ref]) for k in range(3))


def wd_lines(prob, n_nodes, rows, nodes):
    return [None if nodes[r] is None else br.row_lines(prob["pack_d"], prob["cl"], par, prob["n_pops"], n_nodes, nodes=nodes[r])
            for r, par in enumerate(rows)]


def x_wd_bins(prob, lines, edges):
    return bc.reference_rows(lines, len(prob["wd"]), br.ALL, edges)


def summed(x):
    acc = np.zeros(x.shape[1:])
    for xr in x:
        acc = acc + xr
    return acc


class Reference:
    """The honest reference of one (setting, K, Q): a row's nodes and increments are computed once per DISTINCT row (the scripts
    share some three dozen) and kept; nobody changes them.  The edges of the binned calls are the combination's own, from the
    nodes of every distinct row of its scripts."""

    def __init__(self, setting, K, Q):
        self.prob, self.K, self.Q = problem(setting), K, Q
        self.n_nodes = tm.n_nodes_of(self.prob["pack_d"], self.prob["n_pops"], K, Q)
        self._memo = {}
        rows = np.concatenate(self.prob["scripts"])
        _, first = np.unique([r.tobytes() for r in rows], return_index=True)
        self.distinct = rows[np.sort(first)]

    def _per_row(self, what, rows, compute):
        """compute(rows) -> tuple of arrays [row, ...]; memoised per row"""
        miss = [r for r in {r.tobytes(): r for r in rows}.values() if (what, r.tobytes()) not in self._memo]
        if miss:
            miss = np.stack(miss)
            got = compute(miss)
            got = got if isinstance(got, tuple) else (got,)
            for i, r in enumerate(miss):
                self._memo[(what, r.tobytes())] = tuple(g[i] for g in got)
        cols = list(zip(*[self._memo[(what, r.tobytes())] for r in rows]))
        return tuple(np.stack(c) for c in cols)

    def nodes(self, rows):
        miss = [r for r in rows if ("nodes", r.tobytes()) not in self._memo]
        for r, nd in zip(miss, ms_nodes(self.prob, self.K, self.Q, miss)):
            self._memo[("nodes", r.tobytes())] = nd
        return [self._memo[("nodes", r.tobytes())] for r in rows]

    def wd_nodes(self, n_nodes, rows):
        miss = [r for r in rows if ("wdn", n_nodes, r.tobytes()) not in self._memo]
        for r, nd in zip(miss, wd_nodes(self.prob, n_nodes, miss)):
            self._memo[("wdn", n_nodes, r.tobytes())] = nd
        return [self._memo[("wdn", n_nodes, r.tobytes())] for r in rows]

    @functools.lru_cache(maxsize=None)
    def hist_edges(self):
        return hc.quantile_edges(self.nodes(self.distinct), hr.PRIMARY, HIST_BINS)

    @functools.lru_cache(maxsize=None)
    def bins_edges(self):
        return sc.own_edges(self.prob["cl"], self.nodes(self.distinct), hr.PRIMARY, STAR_BINS)

    @functools.lru_cache(maxsize=None)
    def wd_edges(self, n_nodes):
        """(edges [n_wd, 6, WD_BINS + 1], the smallest margin of an edge from a node value, in tolerances)"""
        lines = self.wd_lines(n_nodes, self.distinct)
        edges, _, margin = bc.own_edges(lines, self.distinct, len(self.prob["wd"]), br.ALL)
        return bc.sub_edges(edges, WD_BINS), float(margin.min())

    def moments(self, rows):
        return self._per_row("mom", rows, lambda m: x_moments(self.prob, self.K, self.Q, m, self.nodes(m)))[0]

    def pointwise(self, rows):
        return self._per_row("pw", rows, lambda m: tuple(np.asarray(a) for a in x_pointwise(self.prob, self.K, self.Q, m, self.nodes(m))))

    def hist(self, rows):
        return self._per_row("hist", rows, lambda m: x_hist(self.prob, self.K, self.Q, m, self.nodes(m), self.hist_edges()))[0]

    def bins(self, rows):
        return self._per_row("bins", rows, lambda m: x_bins(self.prob, self.K, self.Q, m, self.nodes(m), self.bins_edges()))[0]

    def resid(self, rows):
        return self._per_row("resid", rows, lambda m: x_resid(self.prob, self.K, self.Q, m, self.nodes(m)))

    def wd_moments(self, n_nodes, rows):
        return self._per_row(("wdm", n_nodes), rows, lambda m: x_wd_moments(self.prob, n_nodes, m, self.wd_nodes(n_nodes, m)))

    def wd_lines(self, n_nodes, rows):
        miss = [r for r in rows if ("wdl", n_nodes, r.tobytes()) not in self._memo]
        if miss:
            for r, ln in zip(miss, wd_lines(self.prob, n_nodes, miss, self.wd_nodes(n_nodes, miss))):
                self._memo[("wdl", n_nodes, r.tobytes())] = ln
        return [self._memo[("wdl", n_nodes, r.tobytes())] for r in rows]

    def wd_bins(self, n_nodes, rows):
        return x_wd_bins(self.prob, self.wd_lines(n_nodes, rows), self.wd_edges(n_nodes)[0])


@functools.lru_cache(maxsize=None)
def reference(setting, K, Q):
    return Reference(setting, K, Q)


# ---- the comparators: one per call, the family's own assertion with the family's own tolerances ------------------------------------
# `got` is what the engine returns for the call; `x` what the matching x_* / Reference method gives for the same rows.
def check_moments(got, x, n_nodes):
    tm.assert_close(got, summed(x), n_nodes)


def check_pointwise(got, x, n_stars):
    """got: (acc, tail [star, TAIL], row_lpd); x: (V, inside, live)"""
    V, inside, _ = x
    inside = np.asarray(inside, dtype=bool)
    pc.assert_acc(got[0], pr.accumulate(V, inside))
    pc.assert_tail(got[1], pr.top_tail(V, inside, TAIL))
    pc.assert_rows(got[2], pr.row_sums(V, inside), n_stars)


def check_hist(got, x, n_nodes, n_stars):
    """got: (star_hist, row_hist)"""
    hc.assert_hist(got[0], got[1], hr.accumulate(x), hr.row_sums(x), n_nodes, n_stars)


def check_bins(got, x, n_nodes, label="star_bins"):
    sc.assert_star_bins(got, summed(x), n_nodes, len(x), label)


def check_resid(got, x, cl, n_nodes, pruning=True):
    """got: (star_resid, row_resid); x: (x, bound, absx)"""
    xs, bound, absx = x
    rc.assert_star_resid(got[0], rr.accumulate(xs), rc.star_atol(bound, absx, n_nodes, pruning))
    rc.assert_row_resid(got[1], rr.row_sums(xs, cl), rc.row_atol(bound, absx, cl["sigma"], n_nodes, pruning))


def check_wd_moments(got, x):
    """x: (x, floor, amp)"""
    wc.assert_accumulated(got, x[0], x[1], "wd_moments")


def check_wd_bins(got, x):
    bc.assert_close(got, bc.summed(x), "wd_bins")


def check_wd_sample(got, x, prob, rows, n_nodes):
    """got: Engine.sample_wd_mass's dict; x: x_wd_moments' tuple for the same rows and n_nodes.  The membership against the
    reference's through wdmoments_check.assert_close; a (row, star) without a finite term draws nothing; every drawn mass is a node
    of the row's OWN grid (its own AGB tip) of its population; the derived values through test_gpu_wdmass.check_derived."""
    import test_gpu_wdmass as tw
    xs = x[0]
    counted = xs[..., wr.ROWS] > 0
    member = np.zeros_like(xs)
    member[..., wr.MEMBER] = got["member"]
    want = np.zeros_like(xs)
    want[..., wr.MEMBER] = xs[..., wr.MEMBER]
    wc.assert_close(member, want, np.zeros_like(xs), "sample_wd_mass member")      # (the MEMBER column's tolerance of b9_wd_moments)
    assert np.array_equal(got["zams"] > 0, counted), "a draw where the reference counts no row, or none where it counts one"
    for r, par in enumerate(rows):
        for k in range(prob["n_pops"]):
            sel = counted[r] & (got["pop"][r] == k)
            if not sel.any():
                continue
            tip = rw.mass_column(prob["pack_d"], par, k)[-1]
            grid = tip + (prob["pack_d"]["m_wd_up"] - tip) / n_nodes * np.arange(1, n_nodes + 1)
            z = got["zams"][r, sel]
            j = np.clip(np.searchsorted(grid, z), 1, n_nodes - 1)
            nearest = np.where(np.abs(grid[j] - z) < np.abs(grid[j - 1] - z), grid[j], grid[j - 1])
            np.testing.assert_allclose(z, nearest, rtol=wd_check.ZAMS_RTOL, atol=0, err_msg="a drawn mass is no node of the row's own grid")
    tw.check_derived(prob["pack_d"], prob["cl"], np.asarray(rows), got)


# ---- the faulty stand-ins --------------------------------------------------------------------------------------------------------
def table_masses(prob, K, par, pop):
    """the primary masses of the row's node table, as numpy_ref.marg_terms forms them (ascending: node index = rank)"""
    imass = rw.mass_column(prob["pack_d"], par, pop)
    out = []
    for e in range(len(imass) - 1):
        d = imass[e + 1] - imass[e]
        if d > 0:
            out += [imass[e] + s * (d / K) for s in range(K)]
    return np.array(out)


def _index_nodes(prob, K, par, star):
    """the primary-node index of every node of a star's (t, m, q, k) in its population's table"""
    t, m, q, k = star
    idx = np.zeros(len(t), dtype=int)
    for pop in np.unique(k):
        tab = table_masses(prob, K, par, int(pop))
        sel = k == pop
        idx[sel] = np.searchsorted(tab, m[sel])
        assert np.array_equal(tab[idx[sel]], m[sel])
    return idx


def _sizes(prob, K, par):
    return [len(table_masses(prob, K, par, pop)) for pop in range(prob["n_pops"])]


def _keep(star, sel):
    return tuple(a[sel] for a in star)


def _join(a, b):
    return tuple(np.concatenate([x, y]) for x, y in zip(a, b))


STAND_INS = ("stale_length", "stale_length_seam", "last_chunk_dropped", "one_interval_invalid", "invalid_repeats", "stale_tip",
             "seed_reads_past_end")
#: the stand-ins that change MS/RGB-stage stars / WD-stage stars of the chain_reduce calls / the b9_wd_* calls
AFFECTS_MS = ("stale_length", "stale_length_seam", "last_chunk_dropped", "one_interval_invalid", "invalid_repeats", "seed_reads_past_end")
AFFECTS_WD_FAMILY = ("one_interval_invalid", "invalid_repeats", "stale_tip")
PRUNE_CUT = 40.0                                    # B9_MARG_CUT: what the walk drops lies this many e-folds below its bound


class _TipShim:
    """base_amd.synth with derive_isochrone's last mass -- the AGB tip numpy_ref.marg_terms_wd starts its steps from -- replaced
    by the tips given per helium value"""

    def __init__(self, tips):
        self.tips = tips

    def __getattr__(self, name):
        return getattr(synth, name)

    def derive_isochrone(self, pack, log_age, feh, y):
        iso = synth.derive_isochrone(pack, log_age, feh, y)
        if iso is None or float(y) not in self.tips:
            return iso
        m = iso[1].copy()
        m[-1] = self.tips[float(y)]
        return iso[0], m, iso[2]


@contextlib.contextmanager
def _stale_tips(prob, par, prev):
    tips = {}
    for pop in range(prob["n_pops"]):
        tips[float(par[abi.P_Y2 if pop else abi.P_Y])] = rw.mass_column(prob["pack_d"], prev, pop)[-1]
    real = numpy_ref.synth
    numpy_ref.synth = _TipShim(tips)
    try:
        yield
    finally:
        numpy_ref.synth = real


def stand_in_ms(kind, prob, K, Q, rows, nodes):
    """(rows', nodes') of the chain_reduce calls under one fault: the honest `nodes` of `rows` changed the way the fault would
    change what a row sees (rows' differs only where a row takes another row's place).
      stale_length          (a) row r is walked with row r - 1's node count where that is larger, the surplus nodes row r - 1's
      stale_length_seam     (b) the same where row r opens a chunk of 32 rows only
      last_chunk_dropped    (c) the last, partial chunk of 64 nodes is not walked
      one_interval_invalid  (d) a row of two common EEPs counts as a row without isochrone
      invalid_repeats       (e) a row without isochrone repeats the row before it
      stale_tip             (f) the WD-stage stars' steps start from row r - 1's AGB tip
      seed_reads_past_end   (g) the seed pass takes every 16th node past the table's end, up to the end of its last chunk, from
                                row r - 1's table: its bound can exceed the star's largest term, and the walk drops what lies
                                PRUNE_CUT e-folds below it"""
    pack_d, cl, n_pops = prob["pack_d"], prob["cl"], prob["n_pops"]
    rows = np.array(rows)
    out = list(nodes)
    ms = np.flatnonzero(np.asarray(cl["stage"]) != abi.STAGE_WD)
    wd = np.flatnonzero(np.asarray(cl["stage"]) == abi.STAGE_WD)
    for r in range(len(rows)):
        cur, prev = nodes[r], nodes[r - 1] if r else None
        if kind == "one_interval_invalid":
            if cur is not None and max(rw.common_range(pack_d, rows[r], p)[1] for p in range(n_pops)) == 2:
                out[r] = None
            continue
        if kind == "invalid_repeats":
            if cur is None and r:
                out[r], rows[r] = out[r - 1], rows[r - 1]
            continue
        if cur is None:
            continue
        new = list(cur)
        if kind == "last_chunk_dropped":
            n = _sizes(prob, K, rows[r])
            for i in ms:
                if len(cur[i][0]):
                    idx = _index_nodes(prob, K, rows[r], cur[i])
                    full = np.array([n[p] // 64 * 64 for p in cur[i][3]])
                    new[i] = _keep(cur[i], idx < full)
        if kind in ("stale_length", "stale_length_seam", "seed_reads_past_end") and prev is not None:
            if kind == "stale_length_seam" and r % CHUNK:
                continue
            n, n_prev = _sizes(prob, K, rows[r]), _sizes(prob, K, rows[r - 1])
            for i in ms:
                if not len(prev[i][0]):
                    continue
                idx = _index_nodes(prob, K, rows[r - 1], prev[i])
                own = np.array([n[p] for p in prev[i][3]])
                if kind == "seed_reads_past_end":
                    end = (own + 63) // 64 * 64
                    stale = (idx >= own) & (idx < end) & (idx % 16 == 0) & (prev[i][2] == 0)
                    if stale.any() and len(cur[i][0]):
                        bound = prev[i][0][stale].max()
                        if bound > cur[i][0].max():
                            new[i] = _keep(cur[i], cur[i][0] >= bound - PRUNE_CUT)
                elif (idx >= own).any():
                    new[i] = _join(cur[i], _keep(prev[i], idx >= own))
        if kind == "stale_tip" and prev is not None and len(wd):
            with _stale_tips(prob, rows[r], rows[r - 1]):
                shifted = mr.star_nodes(pack_d, cl, rows[r], n_pops, K, Q)
            for i in wd:
                new[i] = shifted[i]
        out[r] = new
    return rows, out


def stand_in_wd(kind, prob, n_nodes, rows, nodes):
    """(rows', nodes') of the b9_wd_* calls (wdmoments_ref.star_nodes' nodes) under the faults that reach them"""
    pack_d, cl, n_pops = prob["pack_d"], prob["cl"], prob["n_pops"]
    rows = np.array(rows)
    out = list(nodes)
    for r in range(len(rows)):
        if kind == "one_interval_invalid" and nodes[r] is not None and max(rw.common_range(pack_d, rows[r], p)[1] for p in range(n_pops)) == 2:
            out[r] = None
        if kind == "invalid_repeats" and nodes[r] is None and r:
            out[r], rows[r] = out[r - 1], rows[r - 1]
        if kind == "stale_tip" and nodes[r] is not None and r and nodes[r - 1] is not None:
            with _stale_tips(prob, rows[r], rows[r - 1]):
                out[r] = wr.star_nodes(pack_d, cl, rows[r], n_pops, n_nodes)
    return rows, out


def rejects(check, *args, **kw):
    try:
        check(*args, **kw)
    except AssertionError:
        return True
    return False


# ---- what a device that computed x would hand back: the stand-ins' outputs, and the honest reference's, in the calls' own form ----
MS_CALLS = ("star_moments", "pointwise", "mass_hist", "star_bins", "phot_resid")
WD_CALLS = ("wd_moments", "wd_bins")


def _splice(honest, faulty, changed):
    """the honest per-row arrays with the rows `changed` taken from `faulty` (computed for those rows only)"""
    if isinstance(honest, tuple):
        return tuple(_splice(h, f, changed) for h, f in zip(honest, faulty))
    out = np.array(honest)
    out[changed] = faulty
    return out


def ms_outputs(ref, rows, nodes=None, honest_rows=None):
    """{call: (got-shaped outputs, x)} of the five chain_reduce calls for `rows`: the honest reference's (nodes=None), or those of
    the given nodes (a stand-in's (rows', nodes') with the script's own rows as honest_rows) on the reference's edges; a row the
    stand-in left alone keeps the honest increments."""
    prob, K, Q = ref.prob, ref.K, ref.Q
    base = rows if honest_rows is None else honest_rows
    x = dict(star_moments=ref.moments(base), pointwise=ref.pointwise(base), mass_hist=ref.hist(base), star_bins=ref.bins(base),
             phot_resid=ref.resid(base))
    if nodes is not None:
        hn = ref.nodes(base)
        ch = [r for r in range(len(rows)) if nodes[r] is not hn[r] or not np.array_equal(rows[r], base[r])]
        if ch:
            rw_, nd = np.asarray(rows)[ch], [nodes[r] for r in ch]
            f = dict(star_moments=x_moments(prob, K, Q, rw_, nd), pointwise=tuple(np.asarray(a) for a in x_pointwise(prob, K, Q, rw_, nd)),
                     mass_hist=x_hist(prob, K, Q, rw_, nd, ref.hist_edges()), star_bins=x_bins(prob, K, Q, rw_, nd, ref.bins_edges()),
                     phot_resid=x_resid(prob, K, Q, rw_, nd))
            x = {k: _splice(x[k], f[k], ch) for k in x}
    V, inside, _ = x["pointwise"]
    inside = np.asarray(inside, dtype=bool)
    got = dict(star_moments=summed(x["star_moments"]), pointwise=(pr.accumulate(V, inside), pr.top_tail(V, inside, TAIL), pr.row_sums(V, inside)),
               mass_hist=(hr.accumulate(x["mass_hist"]), hr.row_sums(x["mass_hist"])), star_bins=summed(x["star_bins"]),
               phot_resid=(rr.accumulate(x["phot_resid"][0]), rr.row_sums(x["phot_resid"][0], prob["cl"])))
    return {k: (got[k], x[k]) for k in MS_CALLS}


def wd_outputs(ref, n_nodes, rows, nodes=None):
    """the same for b9_wd_moments and b9_wd_bins"""
    if nodes is None:
        xm, xb = ref.wd_moments(n_nodes, rows), ref.wd_bins(n_nodes, rows)
    else:
        xm = x_wd_moments(ref.prob, n_nodes, rows, nodes)
        xb = x_wd_bins(ref.prob, wd_lines(ref.prob, n_nodes, rows, nodes), ref.wd_edges(n_nodes)[0])
    return dict(wd_moments=(summed(xm[0]), xm), wd_bins=(bc.summed(xb), xb))


def wd_sample_outputs(prob, rows, nodes, seed=0):
    """What b9_sample_wd_mass would hand back if it drew from `nodes` (wdmoments_ref.star_nodes' per row; a stand-in's or the
    honest ones): per (row, WD-stage star) one node drawn with numpy from the star's weights -- its mass, population and derived
    values (0 where the node has no cooling age) -- and the membership; zeros for a row or a star without nodes."""
    rng = np.random.default_rng(seed)
    cl, wd = prob["cl"], prob["wd"]
    names = ("zams", "wd_mass", "prec_log_age", "log_cool_age", "log_teff", "logg", "member")
    out = {k: np.zeros((len(rows), len(wd))) for k in names}
    out["pop"] = np.zeros((len(rows), len(wd)), dtype=np.int32)
    for r, nr in enumerate(nodes):
        for c, (t, m, k, cooled, der) in enumerate(nr or ()):
            if not len(t):
                continue
            mx = t.max()
            L = mx + np.log(np.sum(np.exp(t - mx)))
            w = np.exp(t - L)
            j = rng.choice(len(t), p=w / w.sum())
            out["zams"][r, c], out["pop"][r, c], out["member"][r, c] = m[j], k[j], mr.membership(cl, wd[c], L)
            for q, name in enumerate(names[1:6]):
                out[name][r, c] = der[j, q]
    return out


def check_call(call, got, x, ref, pruning=True):
    """the comparator of `call`: `got` against the reference increments `x`"""
    prob = ref.prob
    if call == "star_moments": check_moments(got, x, ref.n_nodes)
    elif call == "pointwise": check_pointwise(got, x, prob["n_stars"])
    elif call == "mass_hist": check_hist(got, x, ref.n_nodes, prob["n_stars"])
    elif call == "star_bins": check_bins(got, x, ref.n_nodes)
    elif call == "phot_resid": check_resid(got, x, prob["cl"], ref.n_nodes, pruning)
    elif call == "wd_moments": check_wd_moments(got, x)
    elif call == "wd_bins": check_wd_bins(got, x)
    else: raise ValueError(call)


# ---- conditioning: the node terms once more in np.longdouble ---------------------------------------------------------------------
LD = np.longdouble


def terms_longdouble(prob, K, Q, par, nodes, wd_steps=None):
    """Per star of `nodes` (moments_ref.star_nodes' (t, m, q, k) of the row) its terms evaluated again: the node's mass and the
    forward model's fp64 magnitudes taken as given, everything after them -- the Gaussian terms, the prior of the mass, the log
    of the mass step and of the population weight -- in np.longdouble.  wd_steps: the steps of a WD-stage star's grid (8 K)."""
    pack_d, cl, n_pops = prob["pack_d"], prob["cl"], prob["n_pops"]
    wd_steps = wd_steps or 8 * K
    mags = rr.node_mags(pack_d, cl, par, nodes)
    sig, obs = np.asarray(cl["sigma"], dtype=LD), np.asarray(cl["obs"], dtype=LD)
    used = sig > 0
    var = np.where(used, sig * sig, LD(1))
    lam = LD(par[abi.P_LAMBDA])
    lw = [LD(0)] if n_pops == 1 else [np.log(lam), np.log1p(-lam)]
    imass = [rw.mass_column(pack_d, par, pop) for pop in range(n_pops)]
    assert all(np.all(np.diff(m) > 0) for m in imass)
    wd_stage = np.asarray(cl["stage"]) == abi.STAGE_WD
    two_pi = 2 * LD(np.pi) if LD is np.float64 else LD(2) * LD("3.14159265358979323846264338327950288")
    out = []
    for i, (t, m, q, k) in enumerate(nodes):
        if len(t) == 0:
            out.append(np.empty(0, dtype=LD))
            continue
        step = np.empty(len(t), dtype=LD)
        for pop in np.unique(k):
            sel = k == pop
            im = imass[int(pop)]
            if wd_stage[i]:
                step[sel] = (LD(pack_d["m_wd_up"]) - LD(im[-1])) / wd_steps
            else:
                tab = table_masses(prob, K, par, int(pop))
                e = np.searchsorted(tab, m[sel]) // K
                step[sel] = (np.asarray(im[e + 1], dtype=LD) - np.asarray(im[e], dtype=LD)) / K / Q
        lpm = numpy_ref.log_prior_mass(np.asarray(m, dtype=LD), pack_d["m_wd_up"]) + np.log(step)
        d = np.asarray(mags[i], dtype=LD) - obs[i][None, :]
        g = np.where(used[i][None, :], -(np.log(two_pi * var[i])[None, :] + d * d / var[i][None, :]) / 2, LD(0)).sum(axis=1)
        out.append(lpm + g + np.array([lw[int(p)] for p in k], dtype=LD))
    return out


def node_weights(cl, i, t):
    """(p w [node], v) of star i from its terms t, in t's own precision: the membership-weighted node weights every sum of the
    binned and moment calls is made of, and b9_pointwise's value"""
    F = t.dtype.type
    log_fs = -np.sum(np.log(np.asarray(cl["filter_prior_max"], dtype=F) - np.asarray(cl["filter_prior_min"], dtype=F)))
    pm = F(np.asarray(cl["clust_prior"])[i])
    mx = t.max()
    L = mx + np.log(np.sum(np.exp(t - mx)))
    a, b = np.log(pm) + L, np.log1p(-pm) + log_fs
    v = np.maximum(a, b) + np.log1p(np.exp(-np.abs(a - b)))
    return np.exp(a - v) * np.exp(t - L), v


# ---- the record: profiles/ragged_chain_cases.md ---------------------------------------------------------------------------------
def cases_markdown():
    """What the scripts reach, per K and script, on the one-population pack (the two-population pack's cells share the same
    common ranges): `PYTHONPATH=.:tests python tests/ragged_chain.py > profiles/ragged_chain_cases.md`; tests/test_ragged_chain_host.py compares."""
    prob = problem("base4")
    out = ["# Ragged saved-chain scripts: what every script reaches", "",
           "Generated by `PYTHONPATH=.:tests python tests/ragged_chain.py`.  A cell is `inside/across`: how often the transition happens between two rows of",
           "one 32-row chunk, and how often on the row that opens the second chunk (row 32).  The five `chain_reduce` calls --",
           "`b9_pointwise`'s own cap and scratch rule included -- hold 32 rows a chunk at these sizes (asserted from the sources).",
           "`b9_sample_wd_mass`, `b9_wd_moments` and `b9_wd_bins` have drivers of their own that cut chunks of up to 256 rows within 64 MiB",
           "of node tables: at the 63 and 65 nodes of the comparison with the reference a whole script is ONE chunk of theirs, so for",
           "these three calls `across` is the boundary between two CALLS (1 + 32 + rest continued), not between two chunks.  Their own",
           "chunk boundary is crossed, bit for bit and without a reference, at the node count at which the table rule gives 32 rows:",
           ", ".join(f"`{c}` {wd_seam_nodes(c, 4, 1, 25, WD_BINS)} / {wd_seam_nodes(c, 5, 2, 25, WD_BINS)} / {wd_seam_nodes(c, 9, 1, 25, WD_BINS)}" for c in WD_FAMILY)
           + " nodes (4 filters / 5 filters, two populations / 9 filters).", "",
           "Script k is `TOUR + FILLER rotated by k + SEAMS[k] + TAILS[:2 + k mod 4]` of `tests/ragged_chain.py`; a token is the age",
           "index of the row's cell (common EEPs " + ", ".join(f"{a}: {n}" for a, n in enumerate(rw.LADDER_COMMON)) + "), `O` a row outside the grid.", ""]
    for K in (1, 2, 3):
        out += [f"## K = {K}", "", "node chunks per cell: " + ", ".join(
            f"{a}: {rw.n_chunks(prob['pack_d'], rw._cell_row(prob['pack_d'], a, 1), K)}" for a in range(11)), "",
            "| script | rows | seam (rows 31, 32) | " + " | ".join(TRANSITIONS) + " | (n - 1) K mod 64 |", "|" + "---|" * (len(TRANSITIONS) + 4)]
        for k in range(N_SCRIPTS):
            tags = script_tags(prob["pack_d"], prob["scripts"][k], K, 1)
            mods = sorted(int(t[3:]) for t in tags if t.startswith("mod"))
            out.append(f"| {k} | {len(prob['scripts'][k])} | {SEAMS[k][0]} -> {SEAMS[k][1]} | "
                       + " | ".join(f"{tags[t + '@inside']}/{tags[t + '@across']}" for t in TRANSITIONS) + " | " + ", ".join(map(str, mods)) + " |")
        out.append("")
    return "\n".join(out)


if __name__ == "__main__":
    print(cases_markdown())
