"""The fused step's per-block descriptor (StepBlockDev: k_mcmc_step reads pack, catalogue, priors, the block-constant step
fields and the grid's cut from device memory; a launch passes 32 bytes).  Every comparison is BITWISE against the two-launch
runner (b9_tuning.two_launch_steps), which takes everything by value and never sees the descriptor.

Shapes: 300 stars x 8 filters, 3 walkers (the one-step launch; tree_depth = 1 pins it) -- the smallest at which every role of
the launch exists (writers, derivation, heavy-star and hot workgroups) and more than one hot workgroup per walker runs."""
import ctypes as C

import numpy as np
import pytest

from base_amd import abi, engine, mcmc, synth
from conftest import build_problem

pytestmark = pytest.mark.gpu

W = 3
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)

# name -> (build_problem arguments, free parameters)
ONE_POP = (abi.P_LOGAGE, abi.P_FEH, abi.P_MOD, abi.P_ABS)
PACKS = {
    "one_pop_8_filters": (dict(name="dsed", n_filt=8, n_stars=300, wd_frac=0.05), ONE_POP),
    "two_pops_8_filters": (dict(name="parsec", n_filt=8, n_stars=300, n_y=3, n_pops=2, wd_frac=0.05), ONE_POP + (abi.P_LAMBDA,)),
    "one_pop_4_filters": (dict(name="parsec", n_filt=4, n_stars=300, wd_frac=0.05), ONE_POP),
    "long_isochrone": (dict(name="parsec", n_filt=8, n_stars=300, n_feh=3, n_age=4, n_eep=2000), ONE_POP),       # mass_cap > 1024
}
FUSED, TWO_LAUNCH = dict(tree_depth=1), dict(two_launch_steps=1)


def make_engine(pack, stars, priors, options, tuning):
    eng = engine.Engine(pack, stars, priors, options)
    eng.set_tuning(**tuning)
    if "tree_depth" in tuning:
        assert eng.step_depth(W) == 1, "the tuning did not select the one-step launch"
    return eng


def submit(eng, start, lp, free, chol, seed, step0, n_steps, flags, samples, lps, origin):
    """b9_mcmc_run_block with `samples`, `lps` and `row_origin` each wanted or not (engine.mcmc_submit couples the first two)."""
    free = np.ascontiguousarray(free, dtype=np.int32)
    d = len(free)
    k = dict(params=np.array(start, dtype=np.float64), logpost=np.array(lp, dtype=np.float64), free=free,
             ids=np.arange(W, dtype=np.int32), chol=np.ascontiguousarray(chol, dtype=np.float64),
             samples=np.full((n_steps, W, d), np.nan) if samples else None, lps=np.full((n_steps, W), np.nan) if lps else None,
             origin=np.ascontiguousarray(origin, dtype=np.float64) if origin is not None else None,
             rows=np.full((W, abi.row_doubles(d)), np.nan) if origin is not None else None)
    blk = abi.b9_mcmc_block()
    blk.n_walkers, blk.n_free = W, d
    blk.free_idx, blk.chol, blk.walker_ids = k["free"].ctypes.data_as(_ip), k["chol"].ctypes.data_as(_dp), k["ids"].ctypes.data_as(_ip)
    blk.seed, blk.step0, blk.n_steps, blk.flags = int(seed), int(step0), int(n_steps), int(flags)
    blk.params, blk.logpost = k["params"].ctypes.data_as(_dp), k["logpost"].ctypes.data_as(_dp)
    blk.samples = k["samples"].ctypes.data_as(_dp) if samples else None
    blk.lps = k["lps"].ctypes.data_as(_dp) if lps else None
    if origin is not None:
        blk.row_origin, blk.rows = k["origin"].ctypes.data_as(_dp), k["rows"].ctypes.data_as(_dp)
    eng._check(eng.lib.b9_mcmc_run_block(eng._ctx, C.byref(blk)))
    k["blk"], k["pending"] = blk, bool(flags & abi.BLOCK_ASYNC)
    return k


def collect(eng, k):
    if k["pending"]:
        eng._check(eng.lib.b9_mcmc_wait(eng._ctx, C.byref(k["blk"])))
        k["pending"] = False
    return dict(params=k["params"], logpost=k["logpost"], n_acc=int(k["blk"].n_accept), samples=k["samples"], lps=k["lps"], rows=k["rows"])


def same_block(got, want, what):
    for key in ("params", "logpost", "samples", "lps", "rows"):
        assert (got[key] is None) == (want[key] is None), (what, key)
        if got[key] is not None:
            assert not np.isnan(got[key]).any(), (what, key, "not written")
            assert np.array_equal(got[key], want[key]), (what, key)
    assert got["n_acc"] == want["n_acc"], what


# the four continued blocks: steps, proposal factor, seed, samples / lps / row_origin wanted.  A one-step block is the launch
# with has_prev = 0 and derive_next = 0 at once; every slot's descriptor is rewritten (other factor, seed, record pointers)
# while the neighbouring slot's block is in flight.
SEQUENCE = [(7, 0.5, 17, True, True, True), (1, 0.8, 5, False, True, False), (5, 0.3, 99, True, False, True), (2, 0.6, 3, False, False, False)]


def run_sequence(eng, start, lp, free, origin):
    chol0 = np.diag([mcmc.DEFAULT_STEP[int(k)] for k in free])
    out = [collect(eng, submit(eng, start, lp, free, chol0 * 0.5, 11, 0, 2, 0, True, True, origin))]       # from host state
    step0, handles = 2, []
    for n, fac, seed, smp, lps, rows in SEQUENCE:
        if len(handles) == 2:                      # at most two blocks outstanding: collect the older one
            out.append(collect(eng, handles.pop(0)))
        handles.append(submit(eng, start, lp, free, chol0 * fac, seed, step0, n, abi.BLOCK_ASYNC | abi.BLOCK_CONTINUE, smp, lps, origin if rows else None))
        step0 += n
    out += [collect(eng, h) for h in handles]
    return out


@pytest.mark.parametrize("case", list(PACKS))
def test_block_sequence(case):
    """Four consecutive B9_BLOCK_ASYNC | B9_BLOCK_CONTINUE blocks of 7, 1, 5 and 2 steps behind a starting block: positions,
    log-posteriors, accepted counts, chain records and summary rows of every block equal the two-launch runner's.  On the
    two-population pack (k_mcmc_step<8,2>), the 4-filter pack (another instance, other struct padding) and the pack whose
    mass_cap exceeds 1024 (the descriptor's mass_cap / iso_stride reach every role)."""
    kw, free = PACKS[case]
    pack_d, cl, pack, stars, priors, options = build_problem(**kw)
    n_pops = kw.get("n_pops", 1)
    start = synth.walker_params(cl["truth"], W, seed=5, n_pops=n_pops, scale=0.02)
    origin = start[:, list(free)].mean(axis=0)
    runs = []
    for tuning in (FUSED, TWO_LAUNCH):
        eng = make_engine(pack, stars, priors, options, tuning)
        if case == "long_isochrone" and tuning is FUSED:
            assert eng.max_eep() > 1024
        runs.append(run_sequence(eng, start, eng.logpost(start), free, origin))
        eng.close()
    assert len(runs[0]) == len(runs[1]) == 1 + len(SEQUENCE)
    for b, (got, want) in enumerate(zip(*runs)):
        same_block(got, want, f"{case}, block {b}")
    assert sum(r["n_acc"] for r in runs[0]) > 0, "no proposal was accepted: the comparison says nothing"


@pytest.mark.parametrize("change", ["priors", "catalogue"])
def test_reconfiguration(change):
    """Between two blocks of one context the priors change / another catalogue of another size is loaded: the next block (not
    CONTINUE) equals that of a fresh context -- fused and two-launch -- with the new configuration.  A stale descriptor shows here."""
    kw, free = PACKS["one_pop_8_filters"]
    pack_d, cl, pack, stars, priors, options = build_problem(**kw)
    start = synth.walker_params(cl["truth"], W, seed=5, scale=0.02)
    origin = start[:, list(free)].mean(axis=0)
    chol = np.diag([mcmc.DEFAULT_STEP[int(k)] for k in free]) * 0.5
    if change == "priors":
        mean = np.array(cl["truth"], dtype=np.float64)
        mean[abi.P_MOD] += 0.05; mean[abi.P_FEH] -= 0.04
        var = np.zeros(abi.B9_NPARAM)
        var[abi.P_FEH], var[abi.P_MOD], var[abi.P_ABS], var[abi.P_LOGAGE] = 0.1 ** 2, 0.05 ** 2, 0.02 ** 2, 0.2 ** 2
        priors2, stars2 = abi.make_priors(mean, var, pack_d["log_age"][0], pack_d["log_age"][-1]), stars
    else:
        cl2 = synth.make_cluster(pack_d, 777, seed=31, truth=cl["truth"], wd_frac=0.02)
        priors2, stars2 = priors, abi.make_stars(cl2)

    def block(eng, n, seed):
        return collect(eng, submit(eng, start, eng.logpost(start), free, chol, seed, 0, n, 0, True, True, origin))

    eng = make_engine(pack, stars, priors, options, FUSED)
    for n in (5, 3):                               # both slots have held a descriptor of the old configuration
        block(eng, n, 17)
    if change == "priors":
        eng.set_priors(priors2)
    else:
        eng.load_stars(stars2)
    got = block(eng, 6, 23)
    eng.close()
    for tuning in (FUSED, TWO_LAUNCH):
        fresh = make_engine(pack, stars2, priors2, options, tuning)
        same_block(got, block(fresh, 6, 23), f"{change}, fresh context {tuning}")
        fresh.close()
    old = make_engine(pack, stars, priors, options, FUSED)
    before = block(old, 6, 23)
    old.close()
    assert not np.array_equal(before["logpost"], got["logpost"]), "the change of configuration did not change the block"
