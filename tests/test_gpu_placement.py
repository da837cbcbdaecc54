"""A walker's bits do not depend on its launch-mates (tests/placement_check.py; docs/LABNOTES.md section 17): every launch
decision the library keys on the walker count, crossed bit for bit at the smallest shapes where it flips.

  marg_sparse (pieces x walkers <= 5 x CUs: TILE = 2 | 1 of k_star_marg and k_marg_step), marg_star_grid's wsplit (even | odd count),
  b9_logpost's two paths (<= 8 rows in the kernel arguments | copies), make_plan's groups per workgroup, the runner make_tree_plan
  picks (tree | one-step launch), and the walkers grid dimension of the WD-table kernels.

Which form ran is read from the library where it reports it (b9_tuning.plan_debug lines, step_depth, step_tiles_per_block, the
piece count) and restated where it does not (placement_check.wsplit, logpost_path).  No comparison here has a tolerance."""
import time

import numpy as np
import pytest

import placement_check as pc
from base_amd import abi, engine
from test_gpu_instances import _chol, _free, _problem, _start

pytestmark = pytest.mark.gpu

SHAPE = dict(n_feh=3, n_age=5, n_eep=40)
SPLIT_INSTANCES = [(4, 1, 0.0), (16, 2, 0.0), (8, 1, 0.05)]          # (filters, populations, WD-stage fraction), 2000 stars, K = Q = 2


def _report(what, t0, **facts):
    print(f"placement {what}: " + ", ".join(f"{k} {v}" for k, v in facts.items()) + f", {time.perf_counter() - t0:.2f} s")


def _engine(pack, stars, priors, opt, tuning):
    eng = engine.Engine(pack, stars, priors, opt)
    if tuning:
        eng.set_tuning(**tuning)
    return eng


def _marg_case(n_filt, n_pops, n_stars, wd_frac, capfd):
    """The catalogue, the probe rows, an engine factory, the library's CU count, the piece count of the catalogue's plan (None:
    unsplit; the plan prints when it is made, at a context's first evaluation) and tile(W): the star launch's form at W walkers
    by the rules of b9k_marg_split, marg_sparse and launch_star_marg_t, as test_gpu_instances restates them."""
    pack_d, cl, pack, stars, priors = _problem(n_filt, n_pops, n_stars, seed=n_stars + n_filt + n_pops, wd_frac=wd_frac, **SHAPE)
    opt = abi.make_options(abi.MODE_MARGINALISED, n_pops, 2, 2)
    rows = pc.probe_rows(pack_d, cl["truth"], n_pops)
    n_cu = pc.n_cu(capfd)
    probe = engine.Engine(pack, stars, priors, opt)
    pieces, _ = pc.plan_pieces(probe, rows[:1], capfd)
    probe.close()
    n_mc = max(1, (int((np.asarray(cl["stage"]) != abi.STAGE_WD).sum()) + 63) // 64)
    assert (pieces is None) == (n_mc * n_pops >= 512) and (pieces is None or pieces >= n_mc)

    def tile(W):
        if pieces is None:
            return "tiled" if (pc.nfp(n_filt) >= 16 or n_pops == 2) else "scalar"
        return "sparse" if pieces * W <= 5 * n_cu else "split"
    return dict(pack_d=pack_d, cl=cl, rows=rows, n_cu=n_cu, n_pops=n_pops, pieces=pieces, tile=tile,
                make=lambda **tuning: _engine(pack, stars, priors, opt, tuning))


def _thresholds(pieces, n_cu):
    """The largest sparse and the smallest split walker count, and the counts either side of them that keep their side."""
    w_s = (5 * n_cu) // pieces
    if w_s < 2:
        raise pc.NoPower(f"{pieces} pieces on {n_cu} CUs: fewer than two walkers run the sparse form")
    assert pieces * w_s <= 5 * n_cu < pieces * (w_s + 1)
    return w_s, w_s + 1


# ---------------------------------------------------------------------------------------------------------------------------
# marginalised b9_logpost, split catalogue: sparse | split, odd | even, <= 8 | > 8 rows; one context up and down, fresh contexts
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_filt,n_pops,wd_frac", SPLIT_INSTANCES)
def test_marginalised_logpost_split_catalogue(capfd, n_filt, n_pops, wd_frac):
    """2000 stars, K = Q = 2 (with 5 % WD-stage stars: k_marg_wd_table and k_star_marg_wd at every count).  Walker counts 1, 2, 3, 8,
    9 and W_s - 1, W_s, W_d, W_d + 1 about the sparse | split threshold read from the plan's piece count and the library's CU count,
    ascending and then descending on ONE context (buffers sized for the largest count serve the smallest): the probed rows -- first,
    middle and last slot -- equal the same rows evaluated alone, total and every star, bit for bit."""
    t0 = time.perf_counter()
    case = _marg_case(n_filt, n_pops, 2000, wd_frac, capfd)
    if wd_frac:
        assert (np.asarray(case["cl"]["stage"]) == abi.STAGE_WD).sum() >= 50
    pieces, tile = case["pieces"], case["tile"]
    assert pieces is not None, "this catalogue should be split"
    w_s, w_d = _thresholds(pieces, case["n_cu"])
    up = sorted({1, 2, 3, 8, 9, w_s - 1, w_s, w_d, w_d + 1})
    counts = up + up[::-1][1:]
    ev = pc.GpuEvaluator(case["make"], lambda e, W: (tile(W), pc.wsplit(W), pc.logpost_path(W)), None)
    try:
        r = pc.check_logpost(ev, case["rows"], pc.placements(counts, case["rows"].shape[0]))
    finally:
        ev.close()
    got = {f[:2] for f in r["forms"].values()}
    assert got >= {("sparse", 1), ("sparse", 2), ("split", 1), ("split", 2)}, (got, pieces, case["n_cu"])
    assert {f[2] for f in r["forms"].values()} == {"args", "copies"}
    assert tile(w_s) == "sparse" and tile(w_d) == "split"
    _report(f"marginalised logpost {n_filt} filters x {n_pops} populations, wd {wd_frac}", t0, pieces=pieces, CUs=case["n_cu"], W_s=w_s, W_d=w_d, calls=ev.calls)


def test_marginalised_logpost_fresh_context_per_count(capfd):
    """The 4-filter catalogue again with a NEW context for every call, against the W = 1 bits of one reused context."""
    t0 = time.perf_counter()
    case = _marg_case(4, 1, 2000, 0.0, capfd)
    pieces, tile = case["pieces"], case["tile"]
    w_s, w_d = _thresholds(pieces, case["n_cu"])
    form = lambda e, W: (tile(W), pc.wsplit(W), pc.logpost_path(W))          # noqa: E731
    used = pc.GpuEvaluator(case["make"], form, None)
    try:
        one = [used.logpost(case["rows"][r:r + 1]) for r in range(case["rows"].shape[0])]
    finally:
        used.close()
    alone = (np.array([o[0][0] for o in one]), np.stack([o[1][0] for o in one]))
    ev = pc.GpuEvaluator(case["make"], form, None, fresh=True)
    r = pc.check_logpost(ev, case["rows"], pc.placements((1, 2, 3, w_s, w_d, 9, w_d + 1), case["rows"].shape[0]), alone=alone)
    assert {f[:2] for f in r["forms"].values()} >= {("sparse", 1), ("sparse", 2), ("split", 1), ("split", 2)}
    _report("marginalised logpost, fresh context per count", t0, pieces=pieces, W_s=w_s, W_d=w_d, calls=ev.calls)


# ---------------------------------------------------------------------------------------------------------------------------
# marginalised b9_logpost, unsplit: wsplit 1 | 2 | 1
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_filt,n_pops,n_stars,form", [(4, 1, 32768, "scalar"), (16, 2, 16384, "tiled")])
def test_marginalised_logpost_unsplit_walker_groups(capfd, n_filt, n_pops, n_stars, form):
    """An unsplit catalogue (512 chunk-populations) at W = 1, 2, 3: marg_star_grid places the (chunk, walker) workgroups on the
    XCDs with one walker group, two, one.  No oracle: three calls and the W = 1 references."""
    t0 = time.perf_counter()
    case = _marg_case(n_filt, n_pops, n_stars, 0.0, capfd)
    assert case["pieces"] is None and case["tile"](1) == form
    ev = pc.GpuEvaluator(case["make"], lambda e, W: (form, pc.wsplit(W)), None)
    try:
        r = pc.check_logpost(ev, case["rows"], pc.placements((1, 2, 3), case["rows"].shape[0]), expect_forms=[(form, 1), (form, 2)])
    finally:
        ev.close()
    assert r["forms"] == {1: (form, 1), 2: (form, 2), 3: (form, 1)}
    _report(f"marginalised logpost unsplit {form}", t0, stars=n_stars, calls=ev.calls)


# ---------------------------------------------------------------------------------------------------------------------------
# given-mass b9_logpost: 8 | 9 rows, one | several canonical groups per workgroup
# ---------------------------------------------------------------------------------------------------------------------------
def _given_case(n_pops):
    pack_d, cl, pack, stars, priors = _problem(8, n_pops, 3000, seed=3000 + n_pops, wd_frac=0.04, **SHAPE)
    opt = abi.make_options(abi.MODE_GIVEN_MASS, n_pops)
    return dict(pack_d=pack_d, cl=cl, n_pops=n_pops, rows=pc.probe_rows(pack_d, cl["truth"], n_pops),
                make=lambda **tuning: _engine(pack, stars, priors, opt, tuning))


@pytest.mark.parametrize("n_pops", [1, 2])
def test_given_mass_logpost_paths_and_plans(capfd, n_pops):
    """3000 stars x 8 filters with 4 % WD-stage stars at W = 1, 2, 8, 9, 17 (b9_logpost's rows-in-arguments path up to 8, copies
    above) and at the first count where make_plan gives a k_star_like workgroup more than one canonical group (tiles x walkers /
    4096 >= 2 x the group's tiles: 683 walkers for 12 one-tile groups) and the count before it; then down again on the same
    context.  The plans are read from make_plan's own b9_tuning.plan_debug line."""
    t0 = time.perf_counter()
    case = _given_case(n_pops)
    ev = pc.GpuEvaluator(case["make"], lambda e, W: e.plans[W] + (pc.logpost_path(W),), None, capfd=capfd)
    try:
        ev.logpost(case["rows"][:1])
        n_groups, group_tiles = ev.groups
        tiles_hi = n_groups * group_tiles                      # (the catalogue's tiles: between (n_groups - 1) x group_tiles + 1 and this)
        w_big = -(-2 * group_tiles * 4096 // tiles_hi)
        if group_tiles > 4 or w_big > 4096:
            raise pc.NoPower(f"{n_groups} groups of {group_tiles} tiles never share a workgroup at a testable walker count")
        up = [1, 2, 8, 9, 17, w_big - 1, w_big]
        r = pc.check_logpost(ev, case["rows"], pc.placements(up + [17, 9, 8, 2, 1], case["rows"].shape[0]))
    finally:
        ev.close()
    forms = r["forms"]
    assert forms[w_big][0] > 1 and forms[w_big - 1][0] == 1 and forms[17][0] == 1, forms
    assert forms[w_big][1] < forms[17][1], "fewer workgroups per walker once each takes several groups"
    assert forms[8][2] == "args" and forms[9][2] == "copies" and forms[8][:2] == forms[9][:2]
    _report(f"given-mass logpost, {n_pops} population(s)", t0, groups=n_groups, group_tiles=group_tiles, W_big=w_big, plans=forms, calls=ev.calls)


# ---------------------------------------------------------------------------------------------------------------------------
# given-mass sampler: the runner chosen by the walker count alone
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pops", [1, 2])
def test_given_mass_sampler_runner_chosen_by_walker_count(capfd, n_pops):
    """Nothing pinned: ids 0 .. W - 1 for the first W whose step_depth is 1 (k_mcmc_step) against id 5 alone (k_mcmc_tree at
    depth >= 2) and against ids 0, 1; 24 steps, the same seed and step0 on every side."""
    t0 = time.perf_counter()
    case = _given_case(n_pops)
    ev = pc.GpuEvaluator(case["make"], None, lambda e, W: ("depth", e.eng.step_depth(W), "tiles", e.eng.step_tiles_per_block(W)))
    try:
        depth = {W: ev.eng.step_depth(W) for W in range(1, 65)}
        flat = [W for W in sorted(depth) if depth[W] == 1]
        if depth[1] < 2 or not flat or flat[0] <= 5:
            raise pc.NoPower(f"step depths by walker count {depth}: no tree launch for one walker, or no one-step launch between 6 and 64")
        W = flat[0]
        start = _start(case["cl"], W, n_pops, scale=0.1)
        r = pc.check_blocks(ev, start, dict(many=list(range(W)), alone=[5], two=[0, 1]), [("many", "alone"), ("many", "two")],
                            _free(n_pops), _chol(n_pops, 0.1), seed=13, step0=0, n_steps=24)
    finally:
        ev.close()
    assert r["forms"]["many"][1] == 1 and r["forms"]["alone"][1] >= 2, r["forms"]
    _report(f"given-mass sampler, {n_pops} population(s)", t0, W=W, forms=r["forms"], chains=r["compared"])


# ---------------------------------------------------------------------------------------------------------------------------
# marginalised sampler: the fused step and the two-launch step, sparse | split and odd | even
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two_launch", [0, 1])
@pytest.mark.parametrize("n_filt,n_pops", [(4, 1), (16, 2)])
def test_marginalised_sampler_sparse_split_odd_even(capfd, n_filt, n_pops, two_launch):
    """The 2000-star catalogues: blocks of W_s walkers (sparse), W_d = W_s + 1 (split, the other parity), W_d + 1 (split, W_s's
    parity) and id 3 alone, 24 steps: every id the crossed blocks share has the same chain.  Like runner against like runner
    only: the fused step (k_marg_step) in one run, the two-launch step (b9_tuning.two_launch_steps) in the other."""
    t0 = time.perf_counter()
    case = _marg_case(n_filt, n_pops, 2000, 0.0, capfd)
    pieces, tile = case["pieces"], case["tile"]
    w_s, w_d = _thresholds(pieces, case["n_cu"])
    runner = "two-launch" if two_launch else "fused"
    make = (lambda: case["make"](two_launch_steps=1)) if two_launch else case["make"]
    ev = pc.GpuEvaluator(make, None, lambda e, W: (runner, tile(W), pc.wsplit(W)))
    try:
        start = _start(case["cl"], w_d + 1, n_pops, scale=0.1)
        r = pc.check_blocks(ev, start, dict(sparse=list(range(w_s)), split=list(range(w_d)), split1=list(range(w_d + 1)), alone=[3]),
                            [("sparse", "split"), ("split", "split1"), ("split", "alone")], _free(n_pops), _chol(n_pops, 0.3), seed=13, step0=0, n_steps=24)
    finally:
        ev.close()
    f = r["forms"]
    assert f["sparse"][1] == "sparse" and f["split"][1] == "split" and f["split1"][1] == "split" and f["split"][2] != f["split1"][2], f
    _report(f"marginalised sampler {runner}, {n_filt} filters x {n_pops} populations", t0, pieces=pieces, W_s=w_s, W_d=w_d, chains=r["compared"])
