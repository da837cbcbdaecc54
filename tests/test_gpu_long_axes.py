"""Grid axes of 64 to 513 entries through every derivation route on the device (tests/long_axes.py; what its positions, cases
and scripts reach is asserted on the CPU by tests/test_long_axes_host.py).

  R1  the isochrone (k_derive_iso): Engine.derive_isochrone at every position, bit for bit against the reference
  R2  both derive kernels through b9_logpost: rows in kernel arguments (batches of 8, k_derive_iso_rows) and copied (11,
      k_derive_iso); stars ON the row's own mass nodes observed at the reference's magnitudes with sigma = 2^-40
  R3  sampler steps across index 63|64 and 127|128: the one-step launch, the tree launch, the fused step with 8 walkers and one
      or two populations, the fused marginalised step and its two-launch form, against the host twin
  R4  the WD branch on tip columns of 129 and 513 entries, staged whole and as corner columns (tests/test_gpu_wd_seams.py's
      routes on these packs, against tests/wd_ref.py at 50 digits)
  R5  the eight saved-chain reductions over a script hopping between the cells beside the boundaries (tests/ragged_chain.py's
      references and comparators)
  R6  the heavy role's LDS: an age axis just short of the limit runs, one past it is refused on the host
Bracket regimes: n <= 64 a64 (and every other test of the suite); 65 .. 128 a65, a127, a128; > 128 a129, a193, a513, f129,
y129, af129 and the WD packs.  Run with -s: every test prints its figures before it asserts."""
import functools
import math

import numpy as np
import pytest

import long_axes as L
import wd_seams as S
from base_amd import abi, engine

pytestmark = pytest.mark.gpu
PACKS = list(L.SHAPES)


# ---- R1 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PACKS)
def test_r1_isochrone_bit_for_bit_at_every_position(name):
    eng = engine.Engine(abi.make_pack(L.pack(name)))
    n = 0
    for k, p in enumerate(L.positions(name)):
        got = eng.derive_isochrone(p.row)
        assert not np.isnan(got[1]).any() and not np.isnan(got[2]).any()
        n += L.check_isochrone(L.reference(name, k), got)
    if len(L.pack(name)["y"]) > 1:                        # population B reads Y2
        for k, p in enumerate(L.positions(name)):
            row = p.row.copy()
            row[abi.P_Y], row[abi.P_Y2] = row[abi.P_Y2], row[abi.P_Y]
            n += L.check_isochrone(L.reference(name, k), eng.derive_isochrone(row, pop=1))
    eng.close()
    print(f"\nR1 {name}: {len(L.positions(name))} positions, {n} doubles equal to the reference's")
    assert n > 0


# ---- R2 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PACKS)
def test_r2_both_derive_kernels_through_logpost(name):
    """Row k travels in a batch of 8 (slot k mod 8) and in a batch of 11 (slot k mod 11); the catalogue is row k's own.  Every
    per-star value is the star's constant to 1e-12 relative -- one ulp of one magnitude would move it by ~1e-8, asserted once --,
    both batches give the same bits, and outside the grid everything is -inf and nothing NaN."""
    d, P = L.pack(name), L.positions(name)
    eng = engine.Engine(abi.make_pack(d), None, abi.make_priors(), abi.make_options())
    rows = np.array([p.row for p in P])
    worst, moved_seen, n_in = 0.0, False, 0
    k0 = next(k for k in range(len(P)) if L.reference(name, k) is not None)
    eng.load_stars(abi.make_stars(L.node_stars(d, L.reference(name, k0))[0]))      # (a row outside the grid meets the catalogue before it)
    for k, p in enumerate(P):
        iso = L.reference(name, k)
        if iso is not None:
            cl, c0 = L.node_stars(d, iso)
            eng.load_stars(abi.make_stars(cl))
        out = []
        for size in (8, 11):
            idx = [(k - k % size + j) % len(P) for j in range(size)]
            tot, ps = eng.logpost(rows[idx], perstar=True)
            assert not np.isnan(tot).any() and not np.isnan(ps).any()
            out.append((tot[k % size], ps[k % size]))
        assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1]), (name, k)
        if iso is None:
            assert out[0][0] == -math.inf and np.all(out[0][1] == -math.inf), (name, k)
            continue
        n_in += 1
        assert math.isfinite(out[0][0])
        r = float(np.max(np.abs(out[0][1] - c0) / np.abs(c0)))
        worst = max(worst, r)
        assert r <= 1e-12, (name, p.axis, p.node, p.kind, r)
        if not moved_seen:
            s, f = 0, int(np.argmax(np.abs(cl["obs"][0])))
            assert abs(cl["obs"][s, f]) >= 1.0
            cl["obs"][s, f] = math.nextafter(cl["obs"][s, f], math.inf)
            eng.load_stars(abi.make_stars(cl))
            moved = eng.logpost(rows[k][None, :], perstar=True)[1][0][s]
            assert abs(moved - out[0][1][s]) > 1e-10 * abs(out[0][1][s]), (moved, out[0][1][s])
            moved_seen = True
    eng.close()
    print(f"\nR2 {name}: {n_in} rows x 64 stars in batches of 8 and 11, max |value - c0| / |c0| = {worst:.3g}")
    assert moved_seen and n_in >= len(P) - 4


# ---- R3 ----------------------------------------------------------------------------------------------------------------------
def _block(eng, sc, b, lp0, ids=None):
    ids = b["ids"] if ids is None else np.asarray(ids, dtype=np.int32)
    return eng.mcmc_run_block(b["start"][ids], lp0[ids], ids, b["free"], b["chol"], sc.seed, 0, L.STEPS)


def _same_bits(a, b):
    return all(L.same_bits(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]


def _against_logpost(eng, b, chain, ids=None):
    """the largest |recorded log-posterior - b9_logpost at the recorded position| / max(1, |.|)"""
    ids = b["ids"] if ids is None else np.asarray(ids)
    pos = np.repeat(b["start"][ids][None], L.STEPS, axis=0)
    pos[:, :, list(b["free"])] = chain[2]
    want = eng.logpost(pos.reshape(-1, abi.B9_NPARAM)).reshape(chain[3].shape)
    assert not np.isnan(chain[3]).any() and np.all(np.isfinite(want))
    return float(np.max(np.abs(chain[3] - want) / np.maximum(1.0, np.abs(want))))


def _form(eng, sc, b, lp0, twin, label, lp_tol, ids=None):
    """one launch form: positions and accept counts bit for bit the twin's, every recorded log-posterior against b9_logpost,
    a repeated run the same bits"""
    dev = _block(eng, sc, b, lp0, ids)
    err = _against_logpost(eng, b, dev, ids)
    print(f"R3 {sc.name} {label}: accepted {dev[4]} (twin {twin[4]}), positions equal to the twin's "
          f"{L.same_bits(dev[2], twin[2])}, recorded log-posteriors against b9_logpost {err:.3g}")
    assert L.same_bits(dev[2], twin[2]) and L.same_bits(dev[0], twin[0]) and dev[4] == twin[4], label
    assert err <= lp_tol, (label, err)
    assert _same_bits(_block(eng, sc, b, lp0, ids), dev), label + ": a repeated run differs"
    return dev


@pytest.mark.parametrize("sc", L.SCRIPTS, ids=lambda s: s.name)
def test_r3_sampler_steps_across_the_boundaries(sc):
    b = L.build_script(sc)
    eng = engine.Engine(b["pack"], b["stars"], b["priors"], b["options"])
    lp0 = eng.logpost(b["start"])
    assert np.all(np.isfinite(lp0))
    twin = L.run_twin(sc, b, eng.logpost, lp0)
    print()
    if sc.mode == L.GIVEN:
        eng.set_tuning(tree_depth=1)
        assert eng.step_depth(L.WALKERS) == 1
        fused = _form(eng, sc, b, lp0, twin, f"fused step, 8 walkers, {sc.n_pops} population(s)", 0.0)
        c = L.crossings(sc, b, fused[2])
        assert all(c[key] >= 1 for key in L.required_crossings(b))
        if sc.n_pops == 1:
            for w in (0, 1, 2, 3):                            # (starts beside 63|64 and beside 127|128, on either side)
                tw = L.run_twin(sc, b, eng.logpost, lp0, [w])
                assert L.same_bits(tw[2], twin[2][:, w:w + 1])
                eng.set_tuning(tree_depth=1)
                assert eng.step_depth(1) == 1
                one = _form(eng, sc, b, lp0, tw, f"one-step launch, walker {w}", 0.0, [w])
                eng.set_tuning()
                if eng.step_depth(1) < 2:
                    eng.set_tuning(tree_depth=2)
                assert eng.step_depth(1) >= 2
                tree = _form(eng, sc, b, lp0, tw, f"tree launch (depth {eng.step_depth(1)}), walker {w}", 0.0, [w])
                assert _same_bits(tree, one), "tree and one-step launch differ"
            eng.set_tuning(tree_depth=3)
            assert eng.step_depth(L.WALKERS) == 3
            tree8 = _form(eng, sc, b, lp0, twin, "tree launch (depth 3), 8 walkers", 0.0)
            assert _same_bits(tree8, fused)
    else:
        fused = _form(eng, sc, b, lp0, twin, "fused marginalised step", 1e-9)
        eng.set_tuning(two_launch_steps=1)
        two = _form(eng, sc, b, lp0, twin, "two-launch marginalised step", 1e-9)
        assert L.same_bits(fused[2], two[2]) and fused[4] == two[4]
        c = L.crossings(sc, b, fused[2])
        assert all(c[key] >= 1 for key in L.required_crossings(b))
    eng.close()


# ---- R4 ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def seams(monkeypatch):
    """tests/test_gpu_wd_seams.py's routes read their packs and cases from tests/wd_seams.py: hand them these"""
    import test_gpu_wd_seams as W
    monkeypatch.setattr(S, "packs", L.wd_packs)
    monkeypatch.setattr(S, "cases", L.wd_cases)
    monkeypatch.setattr(S, "model", functools.lru_cache(maxsize=None)(S.model.__wrapped__))
    monkeypatch.setattr(W, "_ENG", {})
    yield W
    for e in W._ENG.values():
        e.close()


@pytest.mark.parametrize("name", L.WD_PACKS)
def test_r4_wd_branch_on_long_tip_columns(seams, name):
    """the general form (b9_predict_mags), the lean form alone and among 200 MS stars (b9_logpost per star), the two forms against
    each other, and the 16-node table's derived values (b9_sample_wd_mass) -- 2 x budget + 1 ulp, as everywhere"""
    W = seams
    d, _ = L.wd_pack(name)
    assert (len(d["iso_n_eep"]) > L.TIPS_LDS_MAX) == (name != "w513")
    W.test_r1_general_form_predict_mags(name)
    W.test_r2_lean_form_logpost_alone(name)
    W.test_r2_lean_form_scattered_among_ms_stars(name)
    W.test_r3_lean_form_at_the_general_forms_magnitudes(name)
    W.test_r5_sample_wd_mass_derived_values(name, (0,))


def test_r4_two_populations_on_the_3x3x513_pack(seams, monkeypatch):
    """tests/test_gpu_wd_seams.py's two-population route names its pack: these packs and cases under that name"""
    d, rows = L.wd_pack("w3x3x513")
    cases = [dict(c, pack="B") for c in L.wd_cases() if c["pack"] == "w3x3x513"]
    monkeypatch.setattr(S, "packs", lambda: {"B": (d, rows)})
    monkeypatch.setattr(S, "cases", lambda: cases)
    seams.test_r2_lean_form_two_populations()


@pytest.mark.parametrize("name,n_pops", [("w17x129", 1), ("w3x3x513", 1), ("w3x3x513", 2), ("w513", 1)])
def test_r4_wd_moments_on_long_tip_columns(name, n_pops):
    """b9_wd_moments at 16 nodes (k_wd_node_table's other instantiation) with the pack's seam stars as the WD-stage catalogue:
    all 16 accumulator columns -- rows, membership, the ZAMS mass and the five derived values with their squares, the population
    -- against tests/wdmoments_ref.py through the family's comparator (1e-9 relative, the value columns with their floor)."""
    import wdmoments_check as wc
    import wdmoments_ref as wr
    d, rows = L.wd_pack(name)
    cs = [c for c in L.wd_cases() if c["pack"] == name]
    cl = S.cluster_of(d, cs, np.array([S.case_obs(d, rows[0], c) for c in cs]), 0.03125, 0.875)
    x, floor = wc.reference(d, cl, rows[0][None, :], n_pops, 16)
    eng = engine.Engine(abi.make_pack(d), abi.make_stars(cl), abi.make_priors(), abi.make_options(n_pops=n_pops))
    acc, idx = eng.wd_moments(rows[0][None, :], 16)
    eng.close()
    assert len(idx) == len(cs) and np.all(x[0][:, wr.ROWS] == 1.0)
    assert (x[0][:, wr.MEMBER] > 0.5).sum() >= len(cs) // 2, "the cluster term must carry the stars, or only the field term is compared"
    wc.assert_accumulated(acc, x, floor, f"wd_moments {name}")
    print(f"\nR4 wd_moments {name}, {n_pops} population(s): {len(cs)} WD-stage stars x 16 columns within the family's tolerance")


# ---- R5 ----------------------------------------------------------------------------------------------------------------------
def _chain_engine():
    import ragged_chain as rcn
    return engine.Engine(*rcn.device_args(L.chain_problem(), L.CHAIN_K, L.CHAIN_Q))


def test_r5_saved_chain_reductions_against_their_references():
    import ragged_chain as rcn
    import test_gpu_ragged_chain as T
    ref = L.chain_reference()
    rows, n_nodes = ref.prob["scripts"][0], L.CHAIN_WD_NODES
    want = rcn.ms_outputs(ref, rows)
    want.update(rcn.wd_outputs(ref, n_nodes, rows))
    eng = _chain_engine()
    for name in rcn.MS_CALLS + rcn.WD_CALLS:
        got = T.call(eng, name, ref, rows, n_nodes)
        rcn.check_call(name, got[0] if len(got) == 1 else got, want[name][1], ref)
    g = eng.sample_wd_mass(rows, n_nodes, seed=T.SEED, row0=T.ROW0)
    rcn.check_wd_sample(g, want["wd_moments"][1], ref.prob, rows, n_nodes)
    acc = T.call(eng, "star_moments", ref, rows, n_nodes)[0]
    assert np.all(acc[:, abi.MOM_ROWS] == len(rows))
    eng.close()


def test_r5_every_rows_increment_is_the_row_alone_on_a_fresh_context():
    import test_gpu_ragged_chain as T
    ref = L.chain_reference()
    rows, n_nodes = ref.prob["scripts"][0], L.CHAIN_WD_NODES
    eng = _chain_engine()
    alone = {}
    for j in range(len(rows)):
        fresh = _chain_engine()
        alone[j] = {name: T.call(fresh, name, ref, rows[j], n_nodes, row0=T.ROW0 + j) for name in T.CALLS}
        fresh.close()
    for name in T.CALLS[:-1]:
        whole = T.call(eng, name, ref, rows, n_nodes)
        na = T.N_ACC[name]
        before = T.zeros_like_start(name, whole)
        for j in range(len(rows)):
            one = alone[j][name]
            after = T.call(eng, name, ref, rows[:j + 1], n_nodes, T.zeros_like_start(name, whole))
            if name in T.ADDITIVE:
                assert T.same(after[:na], tuple(x + o for x, o in zip(before, one[:na]))), (name, j)
            else:
                assert T.same(after[:na], T.call(eng, name, ref, rows[j], n_nodes, before)[:na]), (name, j)
            for a, w, o in zip(after[na:], whole[na:], one[na:]):
                assert np.array_equal(a[j], o[0]) and np.array_equal(w[j], o[0]), (name, j)
            before = after[:na]
        assert T.same(before, whole[:na]), name
    batch = T.call(eng, "sample_wd_mass", ref, rows, n_nodes)
    assert (batch[0] > 0).any()
    for j in range(len(rows)):
        assert all(np.array_equal(x[j], o[0]) for x, o in zip(batch, alone[j]["sample_wd_mass"])), j
    eng.close()


# ---- R6 ----------------------------------------------------------------------------------------------------------------------
def _capacity_problem(n_age):
    import ragged_walk as rw
    d = L.capacity_pack(n_age)
    truth = S._row(d, n_age // 2, 0.25, 0, 0.5)
    truth[abi.P_MOD], truth[abi.P_ABS] = 10.2, 0.12
    cl = rw.catalogue(d, truth, 60, 3, 0.05, 2, sigma_scale=30.0)
    start = np.tile(truth, (L.WALKERS, 1))
    la = d["log_age"]
    start[:, abi.P_LOGAGE] += (la[1] - la[0]) * np.linspace(-3.0, 3.0, L.WALKERS)
    from base_amd import synth
    return dict(pack=abi.make_pack(d), stars=abi.make_stars(cl), priors=synth.default_priors(d, truth, 2), start=start,
                options=abi.make_options(n_pops=2), free=np.array([abi.P_LOGAGE, abi.P_FEH, abi.P_MOD, abi.P_ABS, abi.P_LAMBDA], dtype=np.int32),
                chol=np.diag([float(la[1] - la[0]), 2e-3, 2e-3, 1e-3, 2e-2]), ids=np.arange(L.WALKERS, dtype=np.int32))


def _run8(eng, b, seed=5):
    from base_amd import mcmc
    lp0 = eng.logpost(b["start"])
    assert np.all(np.isfinite(lp0))
    args = (b["start"], lp0, b["ids"], b["free"], b["chol"], seed, 0, 8)
    return lp0, args, mcmc.HostBlockRunner(eng.logpost).run(*args)


def test_r6_an_age_axis_past_the_heavy_roles_lds_is_refused_on_the_host():
    """The fused two-population step stages 16 tip columns of n_age doubles (heavy_lds_doubles): b9_mcmc_run_block refuses the
    block -- B9_ERR_CAPACITY, naming the axis -- before it uploads or launches anything (check_step_lds in b9_capi_blocks.cpp,
    ahead of open_block); the refusal's message states the kernel's static LDS, which decides the last axis that fits.  That
    axis runs and matches the twin; the context then loads a small pack and gives a fresh context's bits."""
    import re
    n_over = L.smallest_refused(2)
    b = _capacity_problem(n_over)
    eng = engine.Engine(b["pack"], b["stars"], b["priors"], b["options"])
    eng.set_tuning(tree_depth=1)
    lp0 = eng.logpost(b["start"])
    with pytest.raises(engine.B9Error) as e:
        eng.mcmc_run_block(b["start"], lp0, b["ids"], b["free"], b["chol"], 5, 0, 8)
    msg = str(e.value)
    print(f"\nR6 {n_over} ages: {msg}")
    assert e.value.code == abi.B9_ERR_CAPACITY and f"age axis of {n_over} entries" in msg
    dyn, stat = (int(x) for x in re.search(r"needs (\d+) dynamic \+ (\d+) static bytes", msg).groups())
    assert dyn == L.fused_step_lds_bytes(n_over) and 0 < stat < 16384
    np.testing.assert_array_equal(eng.logpost(b["start"]), lp0)             # nothing is outstanding: the context goes on
    n_fit = n_over
    while L.fused_step_lds_bytes(n_fit) + stat > L.LDS_PER_CU:
        n_fit -= 1
    for n_age, fits in ((n_fit + 1, False), (n_fit, True)):
        b = _capacity_problem(n_age)
        eng.load_pack(b["pack"])
        eng.load_stars(b["stars"])
        eng.set_priors(b["priors"])
        if not fits:
            with pytest.raises(engine.B9Error) as e:
                eng.mcmc_run_block(b["start"], eng.logpost(b["start"]), b["ids"], b["free"], b["chol"], 5, 0, 8)
            assert e.value.code == abi.B9_ERR_CAPACITY
            continue
        lp0, args, twin = _run8(eng, b)
        assert eng.step_depth(L.WALKERS) == 1
        dev = eng.mcmc_run_block(*args)
        print(f"R6 {n_age} ages ({L.fused_step_lds_bytes(n_age)} + {stat} bytes): accepted {dev[4]} (twin {twin[4]})")
        assert L.same_bits(dev[2], twin[2]) and dev[4] == twin[4] and dev[4] > 0
    sc = L.SCRIPTS[1]                                                        # a small pack on the same context: a fresh context's bits
    small = L.build_script(sc)
    eng.load_pack(small["pack"])
    eng.load_stars(small["stars"])
    eng.set_priors(small["priors"])
    fresh = engine.Engine(small["pack"], small["stars"], small["priors"], small["options"])
    fresh.set_tuning(tree_depth=1)
    lp0 = fresh.logpost(small["start"])
    np.testing.assert_array_equal(eng.logpost(small["start"]), lp0)
    assert _same_bits(_block(eng, sc, small, lp0), _block(fresh, sc, small, lp0))
    eng.close()
    fresh.close()


def test_r6_the_two_launch_form_takes_the_axis_the_fused_step_refuses_and_has_a_limit_of_its_own():
    """Given-mass blocks with two launches per step carry the heavy role in k_star_like, one candidate at a time: 8 tip columns of
    n_age doubles under two populations.  The axis the fused step refuses runs in this form (a dynamic request above 64 KB) with
    the twin's bits; the smallest axis past k_star_like's own LDS is refused by the same host-side check, before the block is
    opened -- the context runs the next block without a word about an outstanding one."""
    b = _capacity_problem(L.smallest_refused(2))
    eng = engine.Engine(b["pack"], b["stars"], b["priors"], b["options"])
    eng.set_tuning(two_launch_steps=1)
    assert 64 * 1024 < L.fused_step_lds_bytes(L.smallest_refused(2), 2, 1) < L.LDS_PER_CU - 16384
    lp0, args, twin = _run8(eng, b)
    dev = eng.mcmc_run_block(*args)
    print(f"\nR6 two-launch form, {L.smallest_refused(2)} ages: accepted {dev[4]} (twin {twin[4]})")
    assert L.same_bits(dev[2], twin[2]) and dev[4] == twin[4] and dev[4] > 0
    n_over = L.smallest_refused(1)
    big = _capacity_problem(n_over)
    eng.load_pack(big["pack"])
    eng.load_stars(big["stars"])
    eng.set_priors(big["priors"])
    with pytest.raises(engine.B9Error) as e:           # (b9_logpost would be refused too: the block gets a made-up log-posterior)
        eng.mcmc_run_block(big["start"], np.zeros(L.WALKERS), big["ids"], big["free"], big["chol"], 5, 0, 8)
    print(f"R6 two-launch form, {n_over} ages: {e.value}")
    assert e.value.code == abi.B9_ERR_CAPACITY and f"age axis of {n_over} entries" in str(e.value)
    eng.load_pack(b["pack"])
    eng.load_stars(b["stars"])
    eng.set_priors(b["priors"])
    assert _same_bits(eng.mcmc_run_block(*args), dev)
    eng.close()
