"""Placement independence of a walker: its numbers do not depend on how many walkers share the call or where it sits among them.

The property (docs/LABNOTES.md section 17): a parameter row's log-posterior and per-star
values are the same bits whether it is evaluated alone or as any slot of a batch of any size, and walker id k's chain (recorded
positions, recorded log-posteriors, final state, accepted moves) is the same bits whatever other walkers share its block.  The
launch forms the library picks from the walker count (sparse | split tiles, wsplit 1 | 2, rows in the kernel arguments | copied,
groups per workgroup, tree | one-step runner) must therefore round alike and index alike.

No GPU dependence here.  The checker drives an "evaluator":
    evaluator.logpost(rows) -> (logpost[W], perstar[W, n_stars])
    evaluator.block(rows, lp0, ids, free, chol, seed, step0, n_steps) -> (params, logpost, samples, lps, n_accept)
    evaluator.logpost_form(W), evaluator.block_form(W) -> a hashable label of the launch form a call of W walkers takes
-- the GPU engine (GpuEvaluator; tests/test_gpu_placement.py), a stateless stand-in over the CPU oracle and the host twin of the
sampler, or one of its deliberately placement-dependent mutants (tests/test_placement_host.py).  The comparator is
history_check's (NaN and -inf patterns and the sign of zero count).  The checker also asserts its own power: the two sides of a
cross ran different forms, every chain both accepted and rejected moves, the probe rows differ from each other on at least half
of the stars -- a shape that does not deliver these is refused with "pick another shape", never passed."""
from __future__ import annotations

import re
from typing import Dict, List, NamedTuple, Sequence, Tuple

import numpy as np

from base_amd import abi, synth
from history_check import _bits, first_difference


class PlacementMismatch(AssertionError):
    """kind "logpost": placement = the Placement, who = the probe row; kind "block": placement = (block a, block b), who = walker id."""

    def __init__(self, kind, placement, who, output, where, got, want, forms):
        self.kind, self.placement, self.who, self.output, self.where = kind, placement, who, output, where
        super().__init__(f"{kind}: {placement!r}, {'row' if kind == 'logpost' else 'walker id'} {who}: output {output!r} differs at index {where}: "
                         f"{got!r} here, {want!r} on the other side; forms {forms!r}")


class NoPower(AssertionError):
    def __init__(self, msg):
        super().__init__(msg + " -- pick another shape")


# ---- probe rows and placements --------------------------------------------------------------------------------------------
def probe_rows(pack_d: Dict, truth: np.ndarray, n_pops: int, n_rows: int = 7, seed: int = 17, scale: float = 0.5) -> np.ndarray:
    """n_rows >= 6 distinct parameter rows about the truth.  Row 1 lies outside the grid (log age beyond the pack's axis: the
    -inf pattern), row 2 exactly on a grid node (log age, [Fe/H] and helium on axis values), and with two populations row 3 has
    lambda = 1 and row 4 lambda = 0 (one population's share exactly zero)."""
    assert n_rows >= 6
    rows = synth.walker_params(truth, n_rows, seed=seed, scale=scale, n_pops=n_pops)
    ages, fehs, ys = (np.asarray(pack_d[k], dtype=np.float64) for k in ("log_age", "feh", "y"))
    rows[1, abi.P_LOGAGE] = float(ages[-1]) + 0.5
    rows[2, abi.P_LOGAGE] = float(ages[int(np.argmin(np.abs(ages - truth[abi.P_LOGAGE])))])
    rows[2, abi.P_FEH] = float(fehs[int(np.argmin(np.abs(fehs - truth[abi.P_FEH])))])
    rows[2, abi.P_Y] = float(ys[len(ys) // 2])
    if n_pops == 2:
        rows[2, abi.P_Y2] = float(ys[-1])
        rows[3, abi.P_LAMBDA] = 1.0
        rows[4, abi.P_LAMBDA] = 0.0
    return rows


class Placement(NamedTuple):
    """A batch of W rows: slot p holds probe row probed[p] for every probed position p; slot j elsewhere holds
    fillers[j % len(fillers)].  The fillers are probe rows too, and none of them is a probed row of this batch: a probed row
    occurs exactly once in it, so a read of any other slot changes its value."""
    W: int
    probed: Tuple[Tuple[int, int], ...]          # (position, probe row)
    fillers: Tuple[int, ...]

    def batch_index(self) -> np.ndarray:
        idx = np.array([self.fillers[j % len(self.fillers)] for j in range(self.W)], dtype=np.int64) if self.W > len(self.probed) \
            else np.zeros(self.W, dtype=np.int64)
        for p, r in self.probed:
            idx[p] = r
        return idx


def placements(counts: Sequence[int], n_rows: int) -> List[Placement]:
    """For every walker count, in the given order, one batch with the first, the middle and the last slot probed; which probe
    rows sit there rotates from batch to batch, so every row is probed (at several counts once there are more than a few)."""
    out, k = [], 0
    for W in counts:
        pos = sorted({0, W // 2, W - 1})
        rows = [(k + i) % n_rows for i in range(len(pos))]
        k += len(pos)
        fill = tuple(r for r in range(n_rows) if r not in rows)
        out.append(Placement(int(W), tuple(zip(pos, rows)), fill))
    return out


# ---- b9_logpost -----------------------------------------------------------------------------------------------------------
def _distinct_enough(alone_ps: np.ndarray):
    n = alone_ps.shape[0]
    for a in range(n):
        for b in range(a + 1, n):
            frac = float(np.mean(_bits(alone_ps[a]) != _bits(alone_ps[b])))
            if frac < 0.5:
                raise NoPower(f"probe rows {a} and {b} differ on only {frac:.0%} of the stars: a wrong-slot read could go unseen")


def check_logpost(ev, rows: np.ndarray, places: Sequence[Placement], expect_forms: Sequence = (), alone=None) -> Dict:
    """Every probed row of every placement against the same row evaluated alone (W = 1): total and every star's value, bit for
    bit.  `alone` = (logpost[R], perstar[R, n]) from another evaluator of the same configuration replaces this evaluator's own
    W = 1 calls (a fresh context per call against one reused context).  Returns {"forms": {W: form}, "alone": ...}."""
    R = rows.shape[0]
    if alone is None:
        one = [ev.logpost(rows[r:r + 1]) for r in range(R)]
        alone = (np.array([o[0][0] for o in one]), np.stack([o[1][0] for o in one]))
    a_lp, a_ps = alone
    _distinct_enough(a_ps)
    if not np.any(np.isneginf(a_lp)) or np.isfinite(a_lp).sum() < R - 2:
        raise NoPower(f"the probe rows' log-posteriors {a_lp!r} should hold exactly one row outside the grid")
    forms = {1: ev.logpost_form(1)}
    seen = set()
    if not any(p > 0 for pl in places for p, _ in pl.probed):
        raise NoPower("no placement probes a slot other than the first")
    for pl in places:
        lp, ps = ev.logpost(rows[pl.batch_index()])
        forms[pl.W] = ev.logpost_form(pl.W)          # (after the call: the library reports a plan when it makes it)
        for p, r in pl.probed:
            seen.add(r)
            for name, got, want in (("logpost", lp[p], a_lp[r]), ("perstar", ps[p], a_ps[r])):
                d = first_difference(np.asarray(got), np.asarray(want))
                if d is not None:
                    raise PlacementMismatch("logpost", pl, r, name, (p,) + tuple(d[0]) if d[0] != "shape" else d[0], d[1], d[2],
                                            (forms[pl.W], forms[1]))
    _assert_forms(forms, expect_forms)
    if len(places) >= R and seen != set(range(R)):
        raise NoPower(f"probe rows {sorted(set(range(R)) - seen)} were never probed")
    return dict(forms=forms, alone=alone)


def _assert_forms(forms: Dict, expect_forms: Sequence):
    have = set(forms.values())
    if len(have) < 2:
        raise NoPower(f"every walker count took the same launch form {have!r}: nothing was crossed")
    missing = [f for f in expect_forms if f not in have]
    if missing:
        raise NoPower(f"the launch forms {missing!r} never ran (ran: {forms!r})")


# ---- sampler blocks -------------------------------------------------------------------------------------------------------
def _accepted(start_free: np.ndarray, samples: np.ndarray) -> int:
    """moves of one walker, from its record: steps whose recorded position differs from the one before (the start before the first)"""
    chain = np.concatenate([start_free[None, :], samples])
    return int((_bits(chain[1:]) != _bits(chain[:-1])).any(axis=1).sum())


def check_blocks(ev, start: np.ndarray, blocks: Dict[str, Sequence[int]], crosses: Sequence[Tuple[str, str]], free, chol, seed: int,
                 step0: int, n_steps: int) -> Dict:
    """start[k] is walker id k's starting row.  Every named block -- a list of walker ids, run with explicit walker_ids, the
    fixed proposal factor `chol` and the chain recorded -- is played once; for every cross (a, b) every walker id the two blocks
    share must have the same recorded positions, recorded log-posteriors, final row, final log-posterior and accepted moves in
    both, and the two blocks must have run different forms.  Each walker's starting log-posterior is its row's, evaluated alone."""
    free = np.asarray(free, dtype=np.int32)
    ids_used = sorted({int(k) for ids in blocks.values() for k in ids})
    lp0 = {k: float(ev.logpost(start[k:k + 1])[0][0]) for k in ids_used}
    runs, forms = {}, {}
    for name, ids in blocks.items():
        ids = np.asarray(ids, dtype=np.int32)
        p, l, x, y, n_acc = ev.block(start[ids], np.array([lp0[int(k)] for k in ids]), ids, free, chol, seed, step0, n_steps)
        per = {}
        for j, k in enumerate(ids):
            per[int(k)] = dict(samples=x[:, j].copy(), lps=y[:, j].copy(), params=p[j].copy(), logpost=np.float64(l[j]),
                               accepted=np.int64(_accepted(start[k, free], x[:, j])))
        if sum(int(v["accepted"]) for v in per.values()) != int(n_acc):
            raise AssertionError(f"block {name!r}: {int(n_acc)} accepted moves reported, {sum(int(v['accepted']) for v in per.values())} in its record")
        runs[name], forms[name] = per, ev.block_form(len(ids))
    compared = 0
    for a, b in crosses:
        if forms[a] == forms[b]:
            raise NoPower(f"blocks {a!r} ({len(blocks[a])} walkers) and {b!r} ({len(blocks[b])}) both ran the form {forms[a]!r}")
        common = sorted(set(runs[a]) & set(runs[b]))
        if not common:
            raise NoPower(f"blocks {a!r} and {b!r} share no walker id")
        for k in common:
            for out in ("samples", "lps", "params", "logpost", "accepted"):
                d = first_difference(runs[a][k][out], runs[b][k][out])
                if d is not None:
                    raise PlacementMismatch("block", (a, b), k, out, d[0], d[1], d[2], (forms[a], forms[b]))
            acc = int(runs[a][k]["accepted"])
            if not 0 < acc < n_steps:
                raise NoPower(f"walker id {k} accepted {acc} of {n_steps} moves: a chain that never (or always) moves compares no decision")
            compared += 1
    return dict(forms=forms, compared=compared, runs=runs)


# ---- which form ran: read from the library where it reports it (b9_tuning.plan_debug), restated where it does not ------------------
def nfp(n_filt):
    return 4 if n_filt <= 4 else (8 if n_filt <= 8 else 16)


def problem(n_filt, n_pops, n_stars, seed, wd_frac=0.0, name=None, **pack_kw):
    """The synthetic pack, catalogue and priors of the launch-form tests (test_gpu_instances._problem without its dropped filters)."""
    kw = dict(n_feh=3, n_age=5, n_eep=40)
    kw.update(pack_kw)
    name = name or ("dsed" if n_pops == 2 else "parsec")
    pack_d = synth.make_pack(name, n_filt, n_y=3 if n_pops == 2 else 1, **kw)
    truth = synth.default_params(pack_d)
    cl = synth.make_cluster(pack_d, n_stars, seed=seed, truth=truth, wd_frac=wd_frac, n_pops=n_pops)
    return pack_d, cl, abi.make_pack(pack_d), abi.make_stars(cl), synth.default_priors(pack_d, truth, n_pops)


def n_cu(capfd):
    """The CU count the library plans with (every plan, marg_sparse included, reads the context's), from the given-mass step plan
    it prints under b9_tuning.plan_debug."""
    from base_amd import engine
    _, _, pack, stars, priors = problem(4, 1, 64, seed=1, n_age=6, n_eep=48)
    capfd.readouterr()
    eng = engine.Engine(pack, stars, priors, abi.make_options(abi.MODE_GIVEN_MASS, 1))
    eng.set_tuning(plan_debug=1)
    eng.step_tiles_per_block(1)
    eng.close()
    return int(re.findall(r"b9 step plan: (\d+) CUs", capfd.readouterr().err)[-1])


def plan_pieces(eng, rows, capfd):
    """Evaluate once with the catalogue plan printed (b9_tuning.plan_debug): its piece count, or None when the catalogue is
    not split."""
    capfd.readouterr()
    eng.set_tuning(plan_debug=1)
    out = eng.logpost(rows, perstar=True)
    eng.set_tuning()
    err = capfd.readouterr().err
    m = re.findall(r"\[marg plan\] \d+ chunks.*; (\d+) pieces", err)
    return (int(m[-1]) if m else None), out


def launch_form(eng, rows, W, n_pops, cl, n_cu, capfd):
    n_mc = max(1, (int((np.asarray(cl["stage"]) != abi.STAGE_WD).sum()) + 63) // 64)
    pieces, out = plan_pieces(eng, rows, capfd)
    if n_mc * n_pops >= 512:
        assert pieces is None
        return ("tiled" if (nfp(eng.n_filt) >= 16 or n_pops == 2) else "scalar"), out
    assert pieces is not None and pieces >= n_mc
    return ("sparse" if pieces * W <= 5 * n_cu else "split"), out


# ---- the GPU evaluator ----------------------------------------------------------------------------------------------------
class GpuEvaluator:
    """b9_logpost (per-star output) and b9_mcmc_run_block of one context behind base_amd.engine.Engine -- or, with fresh = True, of
    a new context for every call.  make_engine() builds a configured Engine; logpost_form(evaluator, W) and
    block_form(evaluator, W) name the form a call of W walkers takes.  Under capfd every b9_logpost runs with
    b9_tuning.plan_debug on top of the engine's tuning, and the star-launch plan make_plan prints for a given-mass call is kept in
    plans[W] = (groups per workgroup, workgroups per walker), the catalogue's canonical groups in groups = (number, tiles each)."""

    def __init__(self, make_engine, logpost_form, block_form, capfd=None, fresh=False):
        self.make_engine, self._lform, self._bform, self.capfd, self.fresh = make_engine, logpost_form, block_form, capfd, fresh
        self.eng = None if fresh else self._new()
        self.plans: Dict[int, Tuple[int, int]] = {}
        self.groups = None
        self.calls = 0

    def _new(self):
        eng = self.make_engine()
        if self.capfd is not None:
            eng.update_tuning(plan_debug=1)
        return eng

    def close(self):
        if self.eng is not None:
            self.eng.close()
            self.eng = None

    def _with(self, call):
        eng = self._new() if self.fresh else self.eng
        try:
            if self.capfd is not None:
                self.capfd.readouterr()
            out = call(eng)
            if self.capfd is not None:
                for w, blocks, m, groups, tiles in re.findall(r"b9 logpost plan: (\d+) walkers x (\d+) workgroups \((\d+) groups each\); "
                                                              r"(\d+) canonical groups of (\d+) tiles", self.capfd.readouterr().err):
                    self.plans[int(w)], self.groups = (int(m), int(blocks)), (int(groups), int(tiles))
            self.calls += 1
            return out
        finally:
            if self.fresh:
                eng.close()

    def logpost(self, rows):
        return self._with(lambda e: e.logpost(rows, perstar=True))

    def block(self, rows, lp0, ids, free, chol, seed, step0, n_steps):
        return self._with(lambda e: e.mcmc_run_block(rows, lp0, ids, free, chol, seed, step0, n_steps, True))

    def logpost_form(self, W):
        return self._lform(self, W)

    def block_form(self, W):
        return self._bform(self, W)


def wsplit(W):
    """marg_star_grid: two walker groups across the XCDs for an even walker count, one for an odd one (the library does not report it)"""
    return 2 if W % 2 == 0 else 1


def logpost_path(W):
    """b9_logpost: up to 8 rows ride in the first launch's kernel arguments and the results come back through mapped host
    memory; more are copied (the library does not report it)"""
    return "args" if W <= 8 else "copies"
