"""Grid axes of 64 to 513 entries (tests/long_axes.py), on the CPU: the reference isochrone against the C oracle at every
position, the emulation of the device's counting bracket and the mutants it must tell apart, the sensitivity of the derived
values to the bracket, and what the scripted chains of tests/test_gpu_long_axes.py reach.  Run with -s for the counts
(profiles/long_axes_cases.md records them)."""
import math

import numpy as np
import pytest

import long_axes as L
import oracle
from base_amd import abi, synth

PACKS = list(L.SHAPES)


def test_packs_have_the_shapes_and_stay_strictly_ascending():
    small = L.grid_pack(3, 3, 3, 9, 12)
    like = synth.make_pack("parsec", 3, n_y=3, ragged=True, wd=False, n_feh=3, n_age=9, n_eep=12)
    for k in ("iso_first_eep", "iso_n_eep", "iso_offset"):                       # synth.make_pack's ragged shapes, vectorised
        assert np.array_equal(small[k], like[k]), k
    assert [len(L.pack(n)["log_age"]) for n in PACKS[:7]] == [64, 65, 127, 128, 129, 193, 513]
    shape = lambda n: tuple(len(L.pack(n)[k]) for k in ("feh", "y", "log_age"))
    assert shape("f129") == (129, 1, 2) and shape("y129") == (2, 129, 2) and shape("af129") == (129, 1, 129)
    assert shape("w17x129") == (17, 1, 129) and shape("w3x3x513") == (3, 3, 513) and shape("w513") == (2, 1, 513)
    for n in PACKS:
        d = L.pack(n)
        assert 3 <= d["n_filt"] <= 5 and 8 <= int(d["iso_n_eep"].max()) <= 24 and int(d["iso_n_eep"].min()) >= 2
        for k in ("log_age", "feh", "y"):
            assert np.all(np.diff(d[k]) > 0), (n, k)
    assert 2.0 ** -L.AGE_BITS < 0.01 * np.diff(L.pack("a513")["log_age"]).min()        # the snap moves a node by < 1 % of a cell
    n_tips = {n: len(L.pack(n)["iso_n_eep"]) for n in L.WD_PACKS}
    assert n_tips["w17x129"] > L.TIPS_LDS_MAX and n_tips["w3x3x513"] > L.TIPS_LDS_MAX and n_tips["w513"] == 1026
    assert [L.search_depth(len(L.pack(n)["log_age"])) for n in L.WD_PACKS] == [2, 3, 3] and L.search_depth(64) == 1 and L.search_depth(512) == 2


@pytest.mark.parametrize("name", PACKS)
def test_positions_are_the_stated_ones(name):
    d = L.pack(name)
    for a in L.SHAPES[name][6]:
        ax = d[L.AXIS_KEY[a][0]]
        n = len(ax)
        P = [p for p in L.positions(name) if p.axis == a]
        nodes = sorted({k for k in (0, 1, 62, 63, 64, 65, 126, 127, 128, 129, 191, 192, 193, n - 3, n - 2, n - 1) if 0 <= k < n})
        assert sorted({p.node for p in P}) == nodes
        assert len(P) == 4 * len(nodes) - 1 and sum(p.cell is None for p in P) == 2
        for p in P:
            if p.kind == "on":
                assert p.x == ax[p.node] and p.cell == min(p.node, n - 2)       # (x = ax[n - 1]: cell n - 2, weight 1)
            if p.kind == "below":
                assert p.x < ax[p.node] and math.nextafter(p.x, math.inf) == ax[p.node]
                assert p.cell == (None if p.node == 0 else p.node - 1)
            if p.kind == "above":
                assert p.cell == (None if p.node == n - 1 else p.node)
            if p.kind == "mid":
                assert ax[p.node] < p.x < ax[p.node + 1] and p.cell == p.node
    last = [p for p in L.positions(name) if p.kind == "on" and p.node == n - 1][-1]
    assert L.derive(d, last.row).t["afy".index(last.axis)] == 1.0


@pytest.mark.parametrize("name", PACKS)
def test_reference_equals_the_oracle_at_every_position(name):
    """bit for bit: header, mass column, magnitudes, tip; empty outside the grid"""
    lib, pk = oracle.load(), abi.make_pack(L.pack(name))
    n = 0
    for k, p in enumerate(L.positions(name)):
        want = L.reference(name, k)
        assert (want is None) == (p.cell is None)
        if want is not None:
            assert want.cell["afy".index(p.axis)] == p.cell
        n += L.check_isochrone(want, oracle.derive_isochrone(lib, pk, p.row))
    print(f"\n{name}: {len(L.positions(name))} positions, {n} doubles equal to the oracle's")
    assert n > 0


def _axes_and_positions():
    for name in PACKS:
        d = L.pack(name)
        for a in L.SHAPES[name][6]:
            ax = [float(v) for v in d[L.AXIS_KEY[a][0]]]
            yield name, ax, [p for p in L.positions(name) if p.axis == a]


def test_the_emulated_device_bracket_is_the_stated_one_and_every_mutant_is_rejected():
    rejected = {m: [] for m in L.MUTANTS}
    regimes = set()
    for name, ax, P in _axes_and_positions():
        n = len(ax)
        regimes.add(0 if n <= 64 else (1 if n <= 128 else 2))
        for p in P:
            want = L.bracket(ax, p.x)                    # (outside the grid too: the device brackets before it looks at the range)
            assert L.device_bracket(ax, p.x) == want, (name, p.node, p.kind)
            for m in L.MUTANTS:
                if L.device_bracket(ax, p.x, m) != want:
                    rejected[m].append((name, p.axis, p.node, p.kind))
    assert regimes == {0, 1, 2}
    for m, where in rejected.items():
        print(f"mutant {m}: rejected by {len(where)} positions, first {where[:1]}")
        assert where, m
    # what the issue's own examples say: n = 129 hides the missing third chunk (cell 127 is its last), 193 shows it
    assert not [w for w in rejected["registers_beyond_128"] if w[0] in ("a129", "w17x129")]
    assert [w for w in rejected["registers_beyond_128"] if w[0] == "a193"]


@pytest.mark.parametrize("name", PACKS)
def test_every_position_is_sensitive_to_its_cell(name):
    """Moving the bracket by one cell changes a derived value by more than 1 ulp (or the EEP range) -- towards either neighbour
    at a position inside a cell; at a position on a node or one ulp beside it towards the neighbour that does not share the
    node: the two cells that meet in a node state the same value there, up to the rounding of t."""
    n_checked = 0
    for k, p in enumerate(L.positions(name)):
        if p.cell is None:
            continue
        s = L.cell_sensitivity(name, k)
        n_ax = len(L.pack(name)[L.AXIS_KEY[p.axis][0]])
        far = {"mid": (-1, 1), "on": (1,) if p.node < n_ax - 1 else (-1,), "above": (1,), "below": (-1,)}[p.kind]
        far = [step for step in far if s[step] is not None]
        for step in far:
            assert s[step] > 1.0, (name, p.node, p.kind, step, s)
            n_checked += 1
        if not far:       # no such neighbour: the first cell from just below ax[1], the last cell from ax[n - 2] (or just above)
            assert (p.cell == 0 and p.kind == "below") or (p.cell == n_ax - 2 and p.node == n_ax - 2 and p.kind in ("on", "above")), (name, p)
    assert n_checked >= len(L.positions(name)) - 6


def _count_table(c, b):
    return ", ".join(f"{a} {lab} {dr} {oc} {c[a, lab, dr, oc]}" for a, lab, dr, oc in L.required_crossings(b))


@pytest.mark.parametrize("sc", L.SCRIPTS, ids=lambda s: s.name)
def test_scripted_chains_cross_the_boundaries_in_both_directions(sc):
    """The host twin over the oracle: proposals that crossed index 63|64 and 127|128, upwards and downwards, accepted and
    rejected -- every count at least 1 --, no decision so close that the device could take it the other way, and proposal steps
    of about one cell."""
    b = L.build_script(sc)
    orc = oracle.Oracle(b["pack"], b["stars"], b["priors"], b["options"])
    lp0 = orc.logpost(b["start"])
    assert np.all(np.isfinite(lp0))
    chain = L.run_twin(sc, b, orc.logpost, lp0)
    c = L.crossings(sc, b, chain[2])
    print(f"\n{sc.name}: accepted {chain[4]} of {L.WALKERS * L.STEPS}; {_count_table(c, b)}")
    for key in L.required_crossings(b):
        assert c[key] >= 1, key
    for _, col, ax in b["axes"]:
        step = b["chol"][list(b["free"]).index(col)][list(b["free"]).index(col)]
        assert 0.5 <= step / (ax[1] - ax[0]) <= 1.5
    # margins: |log u - (lp' - lp)| of every decision
    import ragged_walk as rw
    cur, prop = rw.proposals(b["start"], chain[2], list(b["free"]), b["chol"], sc.seed, 0, b["ids"])
    lp_prop = orc.logpost(prop.reshape(-1, abi.B9_NPARAM)).reshape(L.STEPS, L.WALKERS)
    lp_cur = np.concatenate([lp0[None], chain[3][:-1]])
    from base_amd import mcmc
    u = np.stack([mcmc.draws(sc.seed, s, b["ids"], len(b["free"]))[1] for s in range(L.STEPS)])
    fin = np.isfinite(lp_prop)
    margin = np.abs(np.log(u) - (lp_prop - lp_cur))[fin]
    assert margin.min() > 1e-6 * np.abs(lp_prop[fin]).max(), margin.min()


def test_the_saved_chain_script_hops_between_the_cells_beside_the_boundaries():
    prob = L.chain_problem()
    d, rows = prob["pack_d"], prob["scripts"][0]
    la = [float(v) for v in d["log_age"]]
    cells = [L.bracket(la, r[abi.P_LOGAGE]) for r in rows]
    assert tuple(cells) == L.CHAIN_TOKENS and set(cells) == {0, 63, 64, 127, 128, len(la) - 2} and len(rows) == 12
    hops = set(zip(cells, cells[1:]))
    assert {(64, 63), (63, 64), (128, 127), (127, 128)} <= hops
    assert prob["n_stars"] == 120 and len(prob["wd"]) == 18
    for r in rows:                                          # every row has an isochrone: every row re-derives
        assert L.derive(d, r) is not None


def test_wd_cases_sit_on_the_probes_of_every_round():
    import wd_ref as R
    for name in L.WD_PACKS:
        d, rows = L.wd_pack(name)
        na = len(d["log_age"])
        cs = [c for c in L.wd_cases() if c["pack"] == name]
        md = R.Model(R.F64, d, rows[0])
        col0 = list(md.tips.values())[0]
        ms = {c["m1"] for c in cs}
        on = {i for i, t in enumerate(col0) if t in ms}
        j = L.equal_tips_site(na)
        rounds, tail = L.search_path(na, j + 1)                                   # (towards the old end of the column the precursor's
        assert len(rounds) == L.search_depth(na) >= 2                             #  age nears logAge and fewer masses are cases)
        for r in rounds:
            assert len(on & set(r)) >= 5, (name, r, sorted(on))
        assert tail in on and len(on & set(L.search_path(na, na - 2)[0][0])) >= 5
        assert col0[j] == col0[j + 1] and j in rounds[0] and j in on
        tags = set().union(*[c["ref"]["tags"] for c in cs])
        assert {"corner:equal_tips", "corners:mixed(heavy+inside)", "corners:all_heavy", "corners:mixed(inside+light)",
                "corner:on_tip[na-2]", "corner:on_tip[na-1]"} <= tags, sorted(tags)
        print(f"{name}: {len(cs)} cases, tips staged {'whole' if len(d['iso_n_eep']) <= L.TIPS_LDS_MAX else 'as corner columns'}, "
              f"{len(rounds)} rounds")


def test_capacity_limit_follows_heavy_lds_doubles():
    """the smallest age axes whose two-population launches ask for more dynamic LDS than a compute unit has: the fused step
    (two candidates) and k_star_like / the tree launch (one)"""
    n2, n1 = L.smallest_refused(2), L.smallest_refused(1)
    assert len(L.capacity_pack(n2)["iso_n_eep"]) > L.TIPS_LDS_MAX and n1 > n2
    assert 64 * 1024 < L.fused_step_lds_bytes(n2, 2, 1) < L.LDS_PER_CU - 16384        # the two-launch form takes the axis the fused step refuses
    print(f"two populations: fused step {n2 - 1} ages fit ({L.fused_step_lds_bytes(n2 - 1)} bytes), {n2} do not; one candidate {n1 - 1} / {n1}")
