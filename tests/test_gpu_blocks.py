"""The sampler block contract (b9_capi_blocks.cpp: open_block / close_block / collect_block), run through every runner:
tree-speculative at depths 3 and 2, fused and two-launch steps in given-mass mode, fused and two-launch steps in marginalised
mode.  Every comparison is bitwise.  The shape is the smallest at which the frame can go wrong: 300 stars, d = 4, W = 3 and 4
(the int block [free_idx, walker_ids] is packed into 8-byte words, so d + W is tried odd and even), S = 7 steps (the tree's
last launch is a partial one at both depths)."""
import numpy as np
import pytest

from base_amd import abi, engine, hostlib, mcmc, synth
from conftest import build_problem

pytestmark = pytest.mark.gpu

FREE = np.array((abi.P_LOGAGE, abi.P_FEH, abi.P_MOD, abi.P_ABS), dtype=np.int32)
CHOL = np.diag([mcmc.DEFAULT_STEP[int(k)] for k in FREE]) * 0.5
S, SEED = 7, 17
GIVEN, MARG = abi.MODE_GIVEN_MASS, abi.MODE_MARGINALISED
# runner -> (evaluation mode, tuning that selects it, steps per dominant-kernel launch)
RUNNERS = {
    "tree3": (GIVEN, dict(tree_depth=3), 3),
    "tree2": (GIVEN, dict(tree_depth=2), 2),
    "fused": (GIVEN, dict(tree_depth=1), 1),
    "two_launch": (GIVEN, dict(two_launch_steps=1), 1),
    "marg_fused": (MARG, dict(), 1),
    "marg_two_launch": (MARG, dict(two_launch_steps=1), 1),
}
CASES = [(r, W) for r in RUNNERS for W in (3, 4)]


class _Shared:
    """The problem, one engine per runner and one reference block per (runner, W): made once, never changed."""

    def __init__(self):
        self.pack_d, self.cl, self.pack, self.stars, self.priors, _ = build_problem("dsed", 8, n_stars=300, wd_frac=0.05)
        self.truth = synth.default_params(self.pack_d)
        self.engines, self.refs = {}, {}

    def options(self, mode):
        return abi.make_options(mode, 1, 2, 2)

    def new_engine(self, runner):
        mode, tuning, _ = RUNNERS[runner]
        eng = engine.Engine(self.pack, self.stars, self.priors, self.options(mode))
        eng.set_tuning(**tuning)
        return eng

    def engine(self, runner):
        if runner not in self.engines:
            self.engines[runner] = self.new_engine(runner)
        return self.engines[runner]

    def start(self, runner, W):
        start = synth.walker_params(self.truth, W, seed=5, scale=0.02)
        return start, self.engine(runner).logpost(start), start[:, FREE].mean(axis=0)

    def ref(self, runner, W):
        """One synchronous block of S steps with the chain record and the summary rows."""
        if (runner, W) not in self.refs:
            eng = self.engine(runner)
            mode, _, depth = RUNNERS[runner]
            if mode == GIVEN:
                assert eng.step_depth(W) == depth, "the tuning did not select this runner"
            start, lp, origin = self.start(runner, W)
            h = submit(eng, start, lp, S, asynchronous=False, row_origin=origin)
            p, l, x, y, a = eng.mcmc_collect(h)
            blk = h["blk"]
            self.refs[runner, W] = dict(params=p.copy(), logpost=l.copy(), samples=x.copy(), lps=y.copy(), n_acc=a, rows=h["rows"].copy(),
                                        d_rows=blk.d_rows, rows_ready=blk.rows_ready)
        return self.refs[runner, W]

    def close(self):
        for eng in self.engines.values():
            eng.close()


@pytest.fixture(scope="module")
def shared():
    sh = _Shared()
    yield sh
    sh.close()


def submit(eng, start, lp, n_steps, step0=0, **kw):
    return eng.mcmc_submit(start, lp, np.arange(start.shape[0]), FREE, CHOL, SEED, step0, n_steps, **kw)


def same(a, b):
    assert np.array_equal(a, b)


@pytest.mark.parametrize("runner,W", CASES)
def test_block_contract(shared, runner, W):
    eng, ref = shared.engine(runner), shared.ref(runner, W)
    start, lp, origin = shared.start(runner, W)
    # 1. the reference's rows are the host statement of its own chain
    same(ref["rows"], hostlib.summary_rows(ref["samples"], ref["params"], ref["logpost"], origin))
    assert 0 <= ref["n_acc"] <= S * W
    # 2. no chain record, rows: the zero-copy finish of the fused and tree runners
    h = submit(eng, start, lp, S, record=False, asynchronous=False, row_origin=origin)
    p, l, _, _, a = eng.mcmc_collect(h)
    same(p, ref["params"]); same(l, ref["logpost"]); same(h["rows"], ref["rows"])
    assert a == ref["n_acc"]
    # 3. no chain record, no rows
    h = submit(eng, start, lp, S, record=False, asynchronous=False)
    p, l, _, _, a = eng.mcmc_collect(h)
    same(p, ref["params"]); same(l, ref["logpost"])
    assert a == ref["n_acc"]
    # 4. two continued blocks, both enqueued before the first is collected
    for s1 in (3, 1):
        ha = submit(eng, start, lp, s1, asynchronous=True, row_origin=origin)
        hb = submit(eng, start, lp, S - s1, step0=s1, cont=True, asynchronous=True, row_origin=origin)
        pa, la, xa, ya, aa = eng.mcmc_collect(ha)
        pb, lb, xb, yb, ab = eng.mcmc_collect(hb)
        same(np.concatenate([xa, xb]), ref["samples"]); same(np.concatenate([ya, yb]), ref["lps"])
        same(pb, ref["params"]); same(lb, ref["logpost"])
        assert aa + ab == ref["n_acc"]
        same(hb["rows"], hostlib.summary_rows(xb, pb, lb, origin))
    # 5. B9_BLOCK_ROWS_EVENT
    h = submit(eng, start, lp, S, asynchronous=False, row_origin=origin, rows_event=True)
    assert h["blk"].rows_ready and h["blk"].d_rows
    p, l, x, y, a = eng.mcmc_collect(h)
    same(p, ref["params"]); same(l, ref["logpost"]); same(x, ref["samples"]); same(y, ref["lps"]); same(h["rows"], ref["rows"])
    assert a == ref["n_acc"]
    assert not ref["rows_ready"] and ref["d_rows"]          # without the flag


@pytest.mark.parametrize("W", (3, 4))
def test_cross_runner_continue_is_refused(shared, W):
    """6. A fused block cannot be continued by the tree runner; the context runs a fresh block correctly afterwards."""
    eng = shared.new_engine("fused")
    try:
        start, lp, origin = shared.start("fused", W)
        eng.mcmc_collect(submit(eng, start, lp, 3, asynchronous=False))
        eng.set_tuning(tree_depth=3)
        assert eng.step_depth(W) == 3
        with pytest.raises(engine.B9Error) as e:
            submit(eng, start, lp, 4, step0=3, cont=True, asynchronous=False)
        assert e.value.code == abi.B9_ERR_STATE
        ref = shared.ref("tree3", W)
        h = submit(eng, start, lp, S, asynchronous=False, row_origin=origin)
        p, l, x, y, a = eng.mcmc_collect(h)
        same(p, ref["params"]); same(l, ref["logpost"]); same(x, ref["samples"]); same(y, ref["lps"]); same(h["rows"], ref["rows"])
        assert a == ref["n_acc"]
    finally:
        eng.close()


@pytest.mark.parametrize("runner,W", CASES)
def test_timing_brackets(shared, runner, W):
    """7. 19 steps cross the default bracket group of 8 twice and end on a short bracket: the chain does not move, and
    kernel_time_ms counts exactly one launch per dominant-kernel launch of the block."""
    eng, n = shared.engine(runner), 19
    shared.ref(runner, W)                                    # (asserts the runner)
    start, lp, _ = shared.start(runner, W)
    plain = eng.mcmc_collect(submit(eng, start, lp, n, asynchronous=False))
    eng.enable_timing(1)
    try:
        eng.kernel_time_ms(reset=True)
        timed = eng.mcmc_collect(submit(eng, start, lp, n, asynchronous=False))
        ms, launches = eng.kernel_time_ms(reset=True)
    finally:
        eng.enable_timing(0)
    for a, b in zip(plain[:4], timed[:4]):
        same(a, b)
    assert plain[4] == timed[4]
    depth = RUNNERS[runner][2]
    assert launches == -(-n // depth)
    assert ms > 0.0
