"""Sampler blocks that walk across cells whose isochrones differ in length (tests/ragged_walk.py; what its scripted cases reach
is asserted on the CPU by tests/test_ragged_walk_host.py): the fused marginalised step (k_marg_step, whose table builders keep
four table sets per walker and return early behind a table's last chunk) and its two-launch form, the given-mass fused
one-step launch and the tree launch at depth 2 and 3 -- each against the host twin over the engine's own log-posterior, every
distinct recorded state against the oracle, the forms of a mode against each other, a repeated block, and a block cut in two
(B9_BLOCK_CONTINUE) right after a walker moved to a shorter table.  Run with -s, every form prints its largest deviations."""
import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings, strategies as st

import oracle
import ragged_walk as rw
from base_amd import abi, engine, mcmc, synth
from test_gpu_instances import _fused_limit, _mass_cap, _nfp

pytestmark = pytest.mark.gpu


class MemoOracle:
    """the oracle's log-posterior, every distinct row evaluated once (the forms of a case visit the same states)"""

    def __init__(self, b):
        self.orc, self.memo = oracle.Oracle(b["pack"], b["stars"], b["priors"], b["options"]), {}

    def logpost(self, rows):
        new = [r for r in rows if r.tobytes() not in self.memo]
        if new:
            for r, v in zip(new, self.orc.logpost(np.array(new))):
                self.memo[r.tobytes()] = v
        return np.array([self.memo[r.tobytes()] for r in rows])


def _oracle_worst(orc, b, chain):
    """every recorded state against the oracle: the same ones finite, no NaN, the largest |delta| / max(1, |v|)"""
    samples, lps = chain[2], chain[3]
    assert not np.isnan(samples).any() and not np.isnan(lps).any() and not np.isnan(chain[0]).any() and not np.isnan(chain[1]).any()
    rows = np.repeat(b["start"][None], samples.shape[0], axis=0)
    rows[:, :, list(b["free"])] = samples
    want = orc.logpost(rows.reshape(-1, abi.B9_NPARAM)).reshape(lps.shape)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(lps), fin)
    return float(np.max(np.abs(lps[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))))


def _assert_same_bits(a, b):
    for x, y in zip(a[:4], b[:4]):
        np.testing.assert_array_equal(x, y)
    assert a[4] == b[4]


def _form(eng, case, b, lp0, host, orc, label):
    """One launch form of a case: twin, oracle, repeat, and the block cut in two behind a move to a shorter table."""
    args = (b["ids"], b["free"], b["chol"], case.seed)
    dev = eng.mcmc_run_block(b["start"], lp0, *args, 0, case.steps)
    assert dev[4] == host[4] and dev[4] >= 3, (dev[4], host[4])
    rw.compare_chains(dev, host)
    worst = _oracle_worst(orc, b, dev)
    print(f"ragged-walk {case.name} {label}: device against oracle {worst:.3e}")
    assert worst <= 1e-9, worst
    _assert_same_bits(eng.mcmc_run_block(b["start"], lp0, *args, 0, case.steps), dev)
    shorter = rw.walk_tags(rw.block_of(case, b, dev[2]))["shorter"]
    assert shorter and shorter[0] + 1 < case.steps
    cut = shorter[0] + 1
    ha = eng.mcmc_submit(b["start"], lp0, *args, 0, cut, record=True, asynchronous=True)
    hb = eng.mcmc_submit(b["start"], lp0, *args, cut, case.steps - cut, record=True, cont=True, asynchronous=True)
    pa, la, xa, ya, aa = eng.mcmc_collect(ha)
    pb, lb, xb, yb, ab = eng.mcmc_collect(hb)
    np.testing.assert_array_equal(xa[-1], dev[2][cut - 1])
    _assert_same_bits((pb, lb, np.concatenate([xa, xb]), np.concatenate([ya, yb]), aa + ab), dev)
    return dev


@pytest.mark.parametrize("case", rw.MARG_CASES, ids=lambda c: c.name)
def test_marginalised_steps_across_cells_of_different_length(case):
    """k_marg_step and the two-launch step on a scripted case: its node tables grow and shrink by whole chunks, shrink to one
    interval, vanish (no common EEPs, outside the grid, outside the prior) and come back; the companions' rows are taken from
    the wave's tile (runs up to 24 rows) and per lane (25 and more)."""
    b = rw.build_case(case)
    eng = engine.Engine(b["pack"], b["stars"], b["priors"], b["options"])
    assert _mass_cap(eng) <= _fused_limit(_nfp(case.n_filt)), "this pack no longer takes the fused step"
    orc = MemoOracle(b)
    lp0 = eng.logpost(b["start"])
    host = rw.run_twin(case, b, eng.logpost, lp0)
    fused = _form(eng, case, b, lp0, host, orc, "fused")
    eng.set_tuning(two_launch_steps=1)
    two = _form(eng, case, b, lp0, host, orc, "two-launch")
    eng.set_tuning()
    np.testing.assert_array_equal(fused[2], two[2])
    np.testing.assert_array_equal(fused[0], two[0])
    assert fused[4] == two[4]
    print(f"ragged-walk {case.name}: fused against two-launch {float(np.max(np.abs(fused[3] / two[3] - 1.0))):.3e}")
    np.testing.assert_allclose(fused[3], two[3], rtol=1e-12, atol=0)
    np.testing.assert_allclose(fused[1], two[1], rtol=1e-12, atol=0)
    eng.close()


@pytest.mark.parametrize("case", rw.GIVEN_CASES, ids=lambda c: c.name)
def test_given_mass_steps_across_cells_of_different_length(monkeypatch, case):
    """k_mcmc_step (depth 1) and k_mcmc_tree (depth 2 and 3) on a scripted case; the tree launches give the one-step launch's bits."""
    b = rw.build_case(case)
    orc = MemoOracle(b)
    ref = engine.Engine(b["pack"], b["stars"], b["priors"], b["options"])
    lp0 = ref.logpost(b["start"])
    host = rw.run_twin(case, b, ref.logpost, lp0)
    ref.close()
    one = None
    for depth in (1, 2, 3):
        monkeypatch.setenv("B9_TREE_DEPTH", str(depth))
        eng = engine.Engine(b["pack"], b["stars"], b["priors"], b["options"])
        assert eng.step_depth(case.walkers) == depth
        dev = _form(eng, case, b, lp0, host, orc, f"depth {depth}")
        if depth == 1:
            one = dev
        else:
            _assert_same_bits(dev, one)
        eng.close()


_PROBLEMS = {}


def _ladder_problem(seed, n_filt, n_pops):
    key = (seed % 8, n_filt, n_pops)
    if key not in _PROBLEMS:
        pack_d = rw.ladder_pack(n_filt, 3 if n_pops == 2 else 1, key[0], rw.VARIANTS[key[0] % 3])
        truth = rw.truth_row(pack_d)
        cl = rw.catalogue(pack_d, truth, 60, key[0], 0.08, n_pops)
        _PROBLEMS[key] = (pack_d, truth, abi.make_pack(pack_d), abi.make_stars(cl), synth.default_priors(pack_d, truth, n_pops))
    return _PROBLEMS[key]


@settings(max_examples=25, deadline=None, suppress_health_check=[HealthCheck.too_slow])
@given(seed=st.integers(0, 10**6), n_filt=st.sampled_from([3, 8]), K=st.sampled_from([1, 2, 3]), Q=st.sampled_from([1, 2, 4]),
       two_pops=st.booleans(), scale=st.floats(0.3, 30.0))
def test_fused_step_on_ladder_packs_matches_host_twin_and_oracle(seed, n_filt, K, Q, two_pops, scale):
    """The fused marginalised step from random cells of a ladder pack, with steps from a fraction of a cell to several cells."""
    n_pops = 2 if two_pops else 1
    pack_d, truth, pack, stars, priors = _ladder_problem(seed, n_filt, n_pops)
    opt = abi.make_options(abi.MODE_MARGINALISED, n_pops, K, Q)
    eng = engine.Engine(pack, stars, priors, opt)
    assert _mass_cap(eng) <= _fused_limit(_nfp(n_filt))
    rng = np.random.default_rng(seed)
    W = 4
    start = np.tile(truth, (W, 1))
    la = pack_d["log_age"]
    cells = rng.integers(0, 10, W)                            # (cell 10 has no isochrone)
    start[:, abi.P_LOGAGE] = la[cells] + rng.uniform(0.1, 0.9, W) * (la[cells + 1] - la[cells])
    start[:, abi.P_FEH] = rng.uniform(pack_d["feh"][0], pack_d["feh"][-1], W)
    free, chol, ids = rw.free_of(n_pops), rw.chol_of(n_pops, scale), np.arange(W)
    lp0 = eng.logpost(start)
    assert np.all(np.isfinite(lp0))
    host = mcmc.HostBlockRunner(eng.logpost).run(start, lp0, ids, free, chol, seed, 3, 14)
    dev = eng.mcmc_run_block(start, lp0, ids, free, chol, seed, 3, 14)
    rw.compare_chains(dev, host)
    b = dict(pack=pack, stars=stars, priors=priors, options=opt, start=start, free=free)
    assert _oracle_worst(MemoOracle(b), b, dev) <= 1e-9
    eng.close()
