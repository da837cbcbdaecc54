"""A context's results do not depend on its call history (docs/LABNOTES.md section 15).

b9_ctx is a long-lived object with lazily grown, lazily invalidated state (work buffers "grown on demand, never shrunk",
cached occupancy keys, the marginalised catalogue plan, deferred restaging of the stars, two block slots).  Every sequence
below is played on ONE context; after every evaluating step the same step runs alone on a fresh context brought directly to
the current configuration, and every returned array and scalar is compared bit for bit (tests/history_check.py).  The fresh
context is the same code, so the last evaluating step of every sequence is also compared with the CPU oracle (per star, 1e-9
relative) or, for a block, with the host twin as tests/test_gpu_mcmc.py does.  No tolerance enters the history comparison.
"""
import re
import time

import numpy as np
import pytest

import history_check as hc
import oracle
from base_amd import abi, engine, mcmc, synth

pytestmark = pytest.mark.gpu

GIVEN, MARG = hc.GIVEN, hc.MARG
# big: one star above the unsplit threshold test_split_threshold names for NFP 4 and one population (511 chunks are split, the
# 512 chunks of 32705 stars are not); c20k: 79 tiles (sequence 11)
EXTRA = {"big": (32705, 0.0), "c20k": (20000, 0.02)}


@pytest.fixture(scope="module")
def world():
    return hc.World(EXTRA)


def _rel(got, want):
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin)
    return float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin])))) if fin.any() else 0.0


def make_witness(world):
    """the last evaluating step against an independent statement: the oracle per star, or the host twin of a block"""
    def witness(op, args, inp, got, cfg):
        pack, stars, priors = world.pack(cfg.pack)[1], world.stars(cfg.stars)[1], world.priors(cfg.priors)
        opt = abi.make_options(*cfg.options)
        if op == "logpost":
            assert args[1], "a sequence ends in a per-star logpost or a block"
            want_lp, want_ps = oracle.Oracle(pack, stars, priors, opt).logpost(inp["rows"], perstar=True)
            assert _rel(got["perstar"], want_ps) <= 1e-9 and _rel(got["logpost"], want_lp) <= 1e-9
        elif op == "block":
            twin = hc.bring_to(hc.GpuPlayer(), cfg, world)
            try:
                host = mcmc.HostBlockRunner(twin.eng.logpost).run(inp["rows"], got["lp0"], inp["ids"], inp["free"], inp["chol"], inp["seed"],
                                                                  inp["step0"], args[1])
            finally:
                twin.close()
            assert int(got["n_accept"]) == host[4]
            np.testing.assert_allclose(got["samples"], host[2], rtol=1e-12, atol=1e-13)
            np.testing.assert_allclose(got["lps"], host[3], rtol=1e-10)
            want = oracle.Oracle(pack, stars, priors, opt).logpost(got["params"])
            assert _rel(got["logpost"], want) <= 1e-9
        else:
            raise AssertionError(f"the oracle cannot state the sequence's last step {op}")
    return witness


def make_prepare(world):
    """a block's starting log-posteriors, from a helper context of their own: neither context under comparison evaluates
    anything before the block, so the block is the first call that meets a new pack, catalogue, prior or option"""
    def prepare(op, args, inp, cfg):
        if op in ("block", "block_pipelined"):
            helper = hc.bring_to(hc.GpuPlayer(), cfg, world)
            try:
                inp["lp0"] = helper.eng.logpost(inp["rows"])
            finally:
                helper.close()
    return prepare


def run(name, steps, world, on_step=None):
    t0 = time.perf_counter()
    r = hc.play(name, steps, world, hc.GpuPlayer, make_witness(world), prepare=make_prepare(world), on_step=on_step)
    print(f"history sequence {name}: {r['compared']} evaluating steps compared, {time.perf_counter() - t0:.2f} s")
    return r


def test_1_isochrone_length_grows_and_shrinks(world):
    run("1 isochrone length", hc.seq_isochrone_length(), world)


def test_2_filter_width(world):
    run("2 filter width", hc.seq_filter_width(), world)


def test_3_walker_counts(world):
    run("3 walker counts", hc.seq_walker_counts(), world)


@pytest.mark.parametrize("n_pops", [1, 2])
def test_4_heavy_star_share(world, capfd, n_pops):
    """check_ready sizes the heavy-star workgroups per walker as
        est = (WD-stage stars + n_stars / (50 n_pops)) * 2 n_pops;  heavy_parts = clamp((est + 255) / 256, 4, 16)
    (integer divisions; b9_tuning.heavy_parts overrides it).  The fused step's plan line (b9_tuning.plan_debug) prints
    n_walkers x heavy_parts as "N heavy": the library is asked through it, the formula is only the expected value -- one
    population: 6 parts for wd1300 against 4 for the small catalogues."""
    def expected(cat):
        n = world.catalogues[cat][0]
        n_wd = int(np.sum(np.asarray(world.stars(("P8", cat))[0]["stage"]) == abi.STAGE_WD))
        return max(4, min(16, ((n_wd + n // (50 * n_pops)) * 2 * n_pops + 255) // 256))

    def planned(cat):
        cfg = hc.Config()
        for st in [("set_options", GIVEN, n_pops, 2, 2)] + hc.conf("P8", cat) + [("set_tuning", {"tree_depth": 1, "plan_debug": 1})]:
            cfg = cfg.apply(st[0], st[1:])
        capfd.readouterr()
        p = hc.bring_to(hc.GpuPlayer(), cfg, world)
        try:
            inp = hc.make_inputs("block", (1, 1, False, False), cfg, 0, world)
            make_prepare(world)("block", (1, 1, False, False), inp, cfg)
            p.evaluate("block", (1, 1, False, False), inp, cfg, world)
        finally:
            p.close()
        m = re.findall(r"b9 step plan: .* (\d+) walkers x .* \+ (\d+) heavy \+", capfd.readouterr().err)
        assert m, "the fused step printed no plan line"
        walkers, heavy = map(int, m[-1])
        assert walkers == 1
        return heavy
    want = {1: 6, 2: 11}[n_pops]
    assert planned("wd1300") == expected("wd1300") == want
    for cat in ("c65", "c300", "one"):
        assert planned(cat) == expected(cat) == 4
    run(f"4 heavy-star share, {n_pops} population(s)", hc.seq_heavy_share(n_pops), world)


def test_5_modes_and_grids(world):
    run("5 modes and grids", hc.seq_modes_and_grids(), world)


def test_6_split_and_unsplit_marginalised_catalogues(world):
    run("6 split and unsplit", hc.seq_split_unsplit(), world)


def test_7_priors(world):
    seen = []

    def narrowed(i, st, got, cfg):          # the narrowed window: -inf from the used context (the fresh one gave the same bits)
        if cfg.priors[1] == "narrow":
            assert np.all(np.isneginf(got["logpost"])), (i, st)
            if st[0] == "block":
                assert np.all(np.isneginf(got["lps"])) and int(got["n_accept"]) == 0
            seen.append(st[0])
    run("7 priors", hc.seq_priors(), world, on_step=narrowed)
    assert seen == ["logpost", "block"]


SEEDS = (11, 12, 13, 14, 15, 16)


@pytest.mark.parametrize("seed", SEEDS)
def test_8_seeded_random_sequences(world, seed):
    steps = hc.random_sequence(seed, 14)
    try:
        run(f"8 random, seed {seed}", steps, world)
    except BaseException:
        for s in SEEDS:
            print(f"random sequence {s}: {hc.random_sequence(s, 14)!r}")
        raise


def test_11_first_call_of_a_fresh_context(world):
    run("11 first call", hc.seq_first_call(), world)


# ---- 9. rejected calls change nothing -------------------------------------------------------------------------------------
FREE = np.array(mcmc.DEFAULT_FREE, dtype=np.int32)
CHOL = np.diag([3e-4, 2e-3, 8e-4, 6e-4])


def _submit(eng, start, lp, n_steps, step0=0, **kw):
    return eng.mcmc_submit(start, lp, np.arange(start.shape[0]), FREE, CHOL, 17, step0, n_steps, **kw)


def test_9_rejected_calls_change_nothing(world):
    """b9_load_pack and b9_load_stars validate the whole table before they touch the context, b9_set_options before it stores
    the struct, b9_sample_wd_mass before anything: a call refused for its arguments leaves the configuration in force (pinned in
    include/base9_hip.h above b9_load_pack).  After each refusal the next evaluating calls return the bits of before, which are
    also a fresh context's, and a continued block is still accepted (nothing was reconfigured)."""
    cfg = hc.Config()
    for st in hc.conf("P8", "c300") + [("set_options", GIVEN, 1, 2, 2)]:
        cfg = cfg.apply(st[0], st[1:])
    rows = synth.walker_params(world.truth("P8"), 2, seed=3, scale=0.03)
    used, fresh = hc.bring_to(hc.GpuPlayer(), cfg, world), hc.bring_to(hc.GpuPlayer(), cfg, world)
    eng = used.eng
    try:
        want_lp, want_ps = fresh.eng.logpost(rows, perstar=True)
        want_chain = fresh.eng.mcmc_collect(_submit(fresh.eng, rows, want_lp, 12, asynchronous=False))
        pack17 = abi.make_pack(synth.make_pack("parsec", 17, n_feh=4, n_age=8, n_eep=90))

        def bad_stars():
            eng.load_stars(world.bad_stars(cfg.stars))

        def bad_pack():
            eng.load_pack(pack17)

        def bad_options():
            eng.set_options(abi.make_options(GIVEN, 3, 2, 2))

        def bad_wd():
            eng.sample_wd_mass(rows, 0)
        for call, code in ((bad_stars, abi.B9_ERR_INVALID), (bad_pack, abi.B9_ERR_CAPACITY), (bad_options, abi.B9_ERR_INVALID), (bad_wd, abi.B9_ERR_INVALID)):
            lp, ps = eng.logpost(rows, perstar=True)
            assert hc.first_difference(lp, want_lp) is None and hc.first_difference(ps, want_ps) is None
            first = eng.mcmc_collect(_submit(eng, rows, lp, 5, asynchronous=False))
            with pytest.raises(engine.B9Error) as e:
                call()
            assert e.value.code == code, call.__name__
            lp, ps = eng.logpost(rows, perstar=True)
            assert hc.first_difference(lp, want_lp) is None and hc.first_difference(ps, want_ps) is None, call.__name__
            second = eng.mcmc_collect(_submit(eng, rows, lp, 7, step0=5, cont=True, asynchronous=False))      # still continues
            assert hc.first_difference(np.concatenate([first[2], second[2]]), want_chain[2]) is None, call.__name__
            assert hc.first_difference(np.concatenate([first[3], second[3]]), want_chain[3]) is None
            assert hc.first_difference(second[0], want_chain[0]) is None and first[4] + second[4] == want_chain[4]
        assert eng.n_stars == 300 and eng.n_filt == 8
        want = oracle.Oracle(world.pack("P8")[1], world.stars(cfg.stars)[1], world.priors(cfg.priors), abi.make_options(*cfg.options)).logpost(rows, perstar=True)
        assert _rel(ps, want[1]) <= 1e-9
    finally:
        used.close()
        fresh.close()


# ---- 10. B9_BLOCK_CONTINUE across a reconfiguration -----------------------------------------------------------------------
RUNNERS = {"fused": dict(tree_depth=1), "tree": dict(tree_depth=3), "two_launch": dict(two_launch_steps=1)}


@pytest.mark.parametrize("runner", list(RUNNERS))
def test_10_continue_across_a_reconfiguration(world, runner):
    """After a successful b9_load_pack / b9_load_stars / b9_set_priors / b9_set_options the previous block's state carries a
    log-posterior of another posterior: a B9_BLOCK_CONTINUE block is B9_ERR_STATE and the message names the call; a block from
    host state then works and equals a fresh context's.  b9_set_tuning, b9_predict_mags and b9_sample_wd_mass between continued
    blocks stay allowed and the chain equals the unpipelined one bit for bit."""
    cfg = hc.Config()
    for st in hc.conf("P8", "c300") + [("set_options", GIVEN, 1, 2, 2), ("set_tuning", RUNNERS[runner])]:
        cfg = cfg.apply(st[0], st[1:])
    W = 3
    rows = synth.walker_params(world.truth("P8"), W, seed=5, scale=0.03)
    used, fresh = hc.bring_to(hc.GpuPlayer(), cfg, world), hc.bring_to(hc.GpuPlayer(), cfg, world)
    eng = used.eng
    try:
        assert eng.step_depth(W) == (3 if runner == "tree" else 1)
        lp0 = fresh.eng.logpost(rows)
        whole = fresh.eng.mcmc_collect(_submit(fresh.eng, rows, lp0, 13, asynchronous=False))
        head = fresh.eng.mcmc_collect(_submit(fresh.eng, rows, lp0, 6, asynchronous=False))
        reconfigure = {
            "b9_load_pack": lambda: eng.load_pack(world.pack(cfg.pack)[1]),
            "b9_load_stars": lambda: eng.load_stars(world.stars(cfg.stars)[1]),
            "b9_set_priors": lambda: eng.set_priors(world.priors(cfg.priors)),
            "b9_set_options": lambda: eng.set_options(abi.make_options(*cfg.options)),
        }
        for name, call in reconfigure.items():
            a = eng.mcmc_collect(_submit(eng, rows, lp0, 6, asynchronous=False))
            assert hc.first_difference(a[2], head[2]) is None
            call()
            with pytest.raises(engine.B9Error) as e:
                _submit(eng, rows, lp0, 7, step0=6, cont=True, asynchronous=False)
            assert e.value.code == abi.B9_ERR_STATE and name in str(e.value), (name, str(e.value))
            again = eng.mcmc_collect(_submit(eng, rows, lp0, 13, asynchronous=False))          # from host state: a fresh context's block
            for k in range(4):
                assert hc.first_difference(again[k], whole[k]) is None, (name, k)
            assert again[4] == whole[4]
        # allowed between continued blocks
        rng = np.random.default_rng(1)
        ha = _submit(eng, rows, lp0, 6, asynchronous=True)
        a = eng.mcmc_collect(ha)
        eng.set_tuning(**RUNNERS[runner])
        eng.predict_mags(rows[0], rng.uniform(0.3, 6.0, 50), np.zeros(50))
        assert np.all(eng.sample_wd_mass(rows[:2], 65)["zams"] > 0)
        b = eng.mcmc_collect(_submit(eng, rows, lp0, 7, step0=6, cont=True, asynchronous=True))
        assert hc.first_difference(np.concatenate([a[2], b[2]]), whole[2]) is None
        assert hc.first_difference(np.concatenate([a[3], b[3]]), whole[3]) is None
        assert hc.first_difference(b[0], whole[0]) is None and hc.first_difference(b[1], whole[1]) is None
        assert a[4] + b[4] == whole[4]
    finally:
        used.close()
        fresh.close()
