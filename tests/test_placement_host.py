"""The placement checker's own power, on the CPU (tests/placement_check.py; docs/LABNOTES.md section 17).

The checker runs on a stateless stand-in over the CPU oracle (b9_logpost) and the host twin of the sampler
(base_amd.mcmc.HostBlockRunner): every row and every walker is evaluated for itself there, so every cross must pass.  Then on
five stand-ins with ONE placement dependence each -- the kinds a launch form keyed on the walker count can have: each must be
rejected, and at the first placement where its dependence matters, which every test states for itself."""
import numpy as np
import pytest

import oracle
import placement_check as pc
from base_amd import abi, mcmc, synth
from history_check import _bits

N_POPS, N_STARS, N_STEPS = 2, 60, 24
COUNTS = (1, 2, 3, 8, 9, 12, 17)              # the stand-in's "forms": rows in the arguments up to 8 | copied; one | two walker groups
FORM_SWITCH = 8


@pytest.fixture(scope="module")
def case():
    pack_d, cl, pack, stars, priors = pc.problem(8, N_POPS, N_STARS, seed=5, wd_frac=0.05)
    rows = pc.probe_rows(pack_d, cl["truth"], N_POPS)
    opt = abi.make_options(abi.MODE_GIVEN_MASS, N_POPS)
    free = np.array(list(mcmc.DEFAULT_FREE) + [abi.P_Y, abi.P_Y2, abi.P_LAMBDA], dtype=np.int32)
    chol = np.diag([3e-3, 2e-2, 8e-3, 6e-3, 2e-3, 2e-3, 2e-2]) * 0.03         # (every one of the nine chains then both accepts and rejects in 24 steps)
    start = synth.walker_params(cl["truth"], 9, seed=3, scale=0.1, n_pops=N_POPS)
    return dict(orc=oracle.Oracle(pack, stars, priors, opt), rows=rows, places=pc.placements(COUNTS, rows.shape[0]), free=free, chol=chol, start=start)


class OracleEvaluator:
    """What the library would be if a call of W walkers were W calls of one."""

    def __init__(self, orc):
        self.orc = orc

    def logpost(self, rows):
        return self.orc.logpost(rows, perstar=True)

    def draw_ids(self, ids):
        return ids

    def block(self, rows, lp0, ids, free, chol, seed, step0, n_steps):
        return mcmc.HostBlockRunner(lambda r: self.logpost(r)[0]).run(rows, lp0, self.draw_ids(np.asarray(ids)), free, chol, seed, step0, n_steps)

    def logpost_form(self, W):
        return (pc.logpost_path(W), pc.wsplit(W))

    def block_form(self, W):
        return ("tree" if W == 1 else "step", pc.wsplit(W))


BLOCKS = dict(big=list(range(9)), alone=[5], two=[0, 1], six=list(range(6)))
CROSSES = [("big", "two"), ("big", "alone"), ("big", "six")]


def _check_blocks(ev, case):
    return pc.check_blocks(ev, case["start"], BLOCKS, CROSSES, case["free"], case["chol"], seed=13, step0=100, n_steps=N_STEPS)


def test_the_stateless_stand_in_passes(case):
    ev = OracleEvaluator(case["orc"])
    r = pc.check_logpost(ev, case["rows"], case["places"], expect_forms=[("args", 1), ("args", 2), ("copies", 1), ("copies", 2)])
    assert set(r["forms"]) == set(COUNTS)
    b = _check_blocks(ev, case)
    assert b["compared"] == 2 + 1 + 6


def test_placements_probe_every_row_and_never_repeat_a_probed_row(case):
    R = case["rows"].shape[0]
    probed = set()
    for pl in case["places"]:
        idx = pl.batch_index()
        assert idx.shape == (pl.W,) and {p for p, _ in pl.probed} == {0, pl.W // 2, pl.W - 1}
        for p, r in pl.probed:
            assert idx[p] == r and (idx == r).sum() == 1
            probed.add(r)
    assert probed == set(range(R))
    lp = case["orc"].logpost(case["rows"])
    assert np.isneginf(lp[1]) and np.isfinite(np.delete(lp, 1)).all()
    assert case["rows"][3, abi.P_LAMBDA] == 1.0 and case["rows"][4, abi.P_LAMBDA] == 0.0


# ---- the mutants: one placement dependence each ---------------------------------------------------------------------------
def _chunk_sum(v, chunk):
    tot = 0.0
    for i in range(0, len(v), chunk):
        tot += float(np.sum(v[i:i + chunk]))
    return tot


def _chunk(W):
    return max(4, 48 // W)


class ChunkedSum(OracleEvaluator):
    """(a) the per-star terms summed in chunks whose size follows the walker count: a last-bit difference in the total only"""

    def logpost(self, rows):
        lp, ps = super().logpost(rows)
        lp = lp.copy()
        for j in range(len(lp)):
            if np.isfinite(ps[j]).all():
                rest = lp[j] - _chunk_sum(ps[j], len(ps[j]))          # the row's prior part, a function of the row alone
                lp[j] = rest + _chunk_sum(ps[j], _chunk(len(lp)))
        return lp, ps


class FormSwitch(OracleEvaluator):
    """(b) above FORM_SWITCH walkers another form runs, whose values are one ulp up on a handful of stars"""
    stars = (3, 17, 40)

    def logpost(self, rows):
        lp, ps = super().logpost(rows)
        if rows.shape[0] > FORM_SWITCH:
            ps = ps.copy()
            for s in self.stars:
                fin = np.isfinite(ps[:, s])
                ps[fin, s] = np.nextafter(ps[fin, s], np.inf)
        return lp, ps


ISO_PARAMS = [abi.P_LOGAGE, abi.P_FEH, abi.P_Y, abi.P_Y2]


class WrongSlot(OracleEvaluator):
    """(c) walker i > 0 of an even-sized batch read with walker i - 1's derived isochrones"""

    def logpost(self, rows):
        if rows.shape[0] % 2 == 0:
            rows = rows.copy()
            rows[1:, ISO_PARAMS] = rows[:-1, ISO_PARAMS].copy()
        return super().logpost(rows)


class FirstRowsAbsorption(OracleEvaluator):
    """(d) the 9th and later rows evaluated with the first row's absorption"""

    def logpost(self, rows):
        if rows.shape[0] > 8:
            rows = rows.copy()
            rows[8:, abi.P_ABS] = rows[0, abi.P_ABS]
        return super().logpost(rows)


class PositionStream(OracleEvaluator):
    """(e) a walker's proposal stream indexed by its position in the block instead of its id"""

    def draw_ids(self, ids):
        return np.arange(len(ids))


def _first(places, pred):
    for pl in places:
        for p, r in pl.probed:
            if pred(pl, p, r):
                return pl, r
    raise AssertionError("no placement reaches the dependence")


def _expected(name, case):
    rows, places = case["rows"], case["places"]
    lp, ps = case["orc"].logpost(rows, perstar=True)
    inside = np.isfinite(lp)
    if name == "a":          # the first probed row whose chunked sum at this count has other bits than at W = 1
        return _first(places, lambda pl, p, r: inside[r] and np.isfinite(ps[r]).all() and
                      _bits(np.float64(_chunk_sum(ps[r], _chunk(pl.W)))) != _bits(np.float64(_chunk_sum(ps[r], _chunk(1))))) + ("logpost",)
    if name == "b":
        return _first(places, lambda pl, p, r: pl.W > FORM_SWITCH and np.isfinite(ps[r][list(FormSwitch.stars)]).any()) + ("perstar",)
    if name == "c":          # (a row outside the grid is -inf whichever isochrone it is read with, unless the neighbour's lies inside)
        def wrong(pl, p, r):
            left = pl.batch_index()[p - 1] if p > 0 else r
            return pl.W % 2 == 0 and p > 0 and (inside[r] or inside[left]) and np.any(rows[left, ISO_PARAMS] != rows[r, ISO_PARAMS])
        return _first(places, wrong) + ("logpost",)
    if name == "d":
        return _first(places, lambda pl, p, r: pl.W > 8 and p >= 8 and inside[r] and rows[pl.batch_index()[0], abi.P_ABS] != rows[r, abi.P_ABS]) + ("logpost",)
    raise KeyError(name)


@pytest.mark.parametrize("name,mutant", [("a", ChunkedSum), ("b", FormSwitch), ("c", WrongSlot), ("d", FirstRowsAbsorption)],
                         ids=["ChunkedSum", "FormSwitch", "WrongSlot", "FirstRowsAbsorption"])
def test_a_placement_dependent_logpost_is_caught_where_it_first_matters(case, name, mutant):
    want_pl, want_row, want_out = _expected(name, case)
    with pytest.raises(pc.PlacementMismatch) as e:
        pc.check_logpost(mutant(case["orc"]), case["rows"], case["places"])
    assert e.value.kind == "logpost" and e.value.placement == want_pl and e.value.who == want_row, (str(e.value), want_pl, want_row)
    assert e.value.output == want_out
    assert repr(want_pl) in str(e.value)
    # ... and it is this placement's walker count that matters: the placements before it alone pass
    before = case["places"][:case["places"].index(want_pl)]
    if len({pc.logpost_path(pl.W) + str(pc.wsplit(pl.W)) for pl in before} | {"args1"}) >= 2:
        pc.check_logpost(mutant(case["orc"]), case["rows"], before)


def test_a_position_indexed_proposal_stream_is_caught_at_the_first_walker_off_its_position(case):
    # "big" against "two": ids 0 and 1 sit at positions 0 and 1 in both; "big" against "alone": id 5 sits at position 0 of its own block
    assert all(BLOCKS[a][:len(BLOCKS[b])] == BLOCKS[b] for a, b in CROSSES[:1]) and BLOCKS["alone"] == [5]
    with pytest.raises(pc.PlacementMismatch) as e:
        _check_blocks(PositionStream(case["orc"]), case)
    assert e.value.kind == "block" and e.value.placement == ("big", "alone") and e.value.who == 5 and e.value.output == "samples"


def test_power_conditions_are_asserted(case):
    ev = OracleEvaluator(case["orc"])
    with pytest.raises(pc.NoPower, match="pick another shape"):          # one form only
        pc.check_logpost(ev, case["rows"], pc.placements((1, 3, 5, 7), 7))
    same = np.repeat(case["rows"][:1], 7, axis=0)
    same[1] = case["rows"][1]
    with pytest.raises(pc.NoPower, match="differ on only"):
        pc.check_logpost(ev, same, case["places"])
    with pytest.raises(pc.NoPower, match="both ran the form"):
        pc.check_blocks(ev, case["start"], dict(a=[0, 1, 2], b=[0, 1, 2, 3, 4]), [("a", "b")], case["free"], case["chol"], 13, 100, N_STEPS)
    with pytest.raises(pc.NoPower, match="accepted 0 of"):                # a proposal too wide to be accepted
        pc.check_blocks(ev, case["start"], dict(a=[0, 1], b=[0]), [("a", "b")], case["free"], case["chol"] * 300, 13, 100, N_STEPS)
    with pytest.raises(pc.NoPower, match="accepted 24 of"):               # ... and too narrow to be refused
        pc.check_blocks(ev, case["start"], dict(a=[0, 1], b=[0]), [("a", "b")], case["free"], case["chol"] * 1e-6, 13, 100, N_STEPS)
