"""The scripted ragged-walk cases (tests/ragged_walk.py) on the CPU: what the cases must reach for the GPU comparison in
tests/test_gpu_ragged_walk.py to test anything, asserted against the chain the host twin makes of the ORACLE's log-posterior;
and that comparison's own power, in the idiom of tests/test_history_host.py: three evaluators with one fault each, run through
the same twin, must be rejected by the GPU test's comparator at the step where the fault first matters.

The conditions are properties of the inputs (packs, catalogues, seeds, scales), not of the code under test: a seed or scale
that misses one is replaced here, on the CPU."""
import collections

import numpy as np
import pytest

import oracle
import ragged_walk as rw
from base_amd import abi

_CHAINS = {}


def chain_of(case):
    """(build, lp0, the host twin's chain over the oracle, every evaluation it made, the tagger's output); once per process"""
    if case.name not in _CHAINS:
        b = rw.build_case(case)
        orc = oracle.Oracle(b["pack"], b["stars"], b["priors"], b["options"])
        lp0 = orc.logpost(b["start"])
        log = rw.Logged(orc.logpost)
        chain = rw.run_twin(case, b, log, lp0)
        _CHAINS[case.name] = (b, lp0, chain, log, rw.walk_tags(rw.block_of(case, b, chain[2])))
    return _CHAINS[case.name]


def _sum(cases, key):
    total = collections.Counter()
    for c in cases:
        total.update(chain_of(c)[4][key])
    return total


# ---- the inputs reach what they were built to reach ---------------------------------------------------------------------------
def test_the_ladder_pack_has_every_rung():
    for n_y, variant in ((1, "base"), (3, "flat"), (1, "wdragged")):
        d = rw.ladder_pack(8, n_y, seed=3, variant=variant)
        assert d["iso_n_eep"].max() <= 160
        counts = set()
        for a in range(11):
            for f in range(3):
                row = rw._cell_row(d, a, f)
                valid, n, lo = rw.common_range(d, row)
                assert valid == (n >= 2)
                for K in (1, 2, 3):
                    assert rw.n_chunks(d, row, K) == (-(-(n - 1) * K // 64) if valid else 0)
                counts.add(n)
                (ia, i_f, iy), _ = rw.cell_of(d, row)
                firsts = {int(d["iso_first_eep"][((i_f + df) * n_y + iy) * 12 + ia + da]) for df in (0, 1) for da in (0, 1)}
                assert len(firsts) > 1, "the corners of a cell share one first EEP"
        assert counts == {158, 66, 65, 64, 34, 33, 32, 3, 2, 1}
        for K in (1, 2, 3):                       # (n - 1) K just below, on and just above a multiple of 64
            nodes = {(n - 1) * K for n in counts}
            assert any(v % 64 == 0 for v in nodes) and any(v % 64 == 64 - K for v in nodes) and any(v % 64 == K for v in nodes), (K, nodes)
        if variant == "flat":
            mass = rw.mass_column(d, rw._cell_row(d, 1, 1))
            assert (np.diff(mass) == 0).sum() == 1
        assert ("wc_n_age" in d) == (variant == "wdragged")
        assert [rw.n_chunks(d, rw._cell_row(d, a, 1), 2) for a in range(11)] == [2, 2, 3, 5, 5, 2, 1, 1, 1, 1, 0]


def test_companion_runs_restate_the_bracket():
    """companion_runs against a per-node loop written out in full"""
    d = rw.ladder_pack(3, 1, seed=1)
    mass = rw.mass_column(d, rw._cell_row(d, 3, 1))
    K, Q = 2, 4
    got = rw.companion_runs(mass, K, Q)
    n = len(mass)
    for c in range(((n - 1) * K + 63) // 64):
        for j in range(1, Q):
            los = []
            for node in range(c * 64, min(c * 64 + 64, (n - 1) * K)):
                e, s = divmod(node, K)
                m2 = (j / Q) * (mass[e] + s * (mass[e + 1] - mass[e]) / K)
                if m2 >= mass[0]:
                    los.append(max(i for i in range(n - 1) if mass[i] <= m2))
            assert got[(c, j)] == (max(los) - min(los) + 2 if los else 0)


@pytest.mark.parametrize("case", rw.CASES, ids=lambda c: c.name)
def test_every_case_moves_is_refused_and_is_decided_clearly(case):
    b, lp0, chain, log, tags = chain_of(case)
    assert case.walkers <= 5 and case.steps <= 40 and len(b["cl"]["mass1"]) <= 200 and b["pack_d"]["iso_n_eep"].max() <= 160
    assert np.all(np.isfinite(lp0))
    assert 0.2 <= tags["n_invalid"] / tags["n_steps"] <= 0.8, tags["n_invalid"]
    assert tags["n_accept"] >= 3 and tags["n_accept"] == chain[4]
    # no rounding difference of a device turns a decision
    assert rw.decision_margins(case, b, lp0, chain, log).min() > 1e-6
    # the catalogue is the cluster's: at the truth the cluster term is the larger one for 80 % of the stars
    orc = oracle.Oracle(b["pack"], b["stars"], b["priors"], b["options"])
    assert rw.dominance(orc.logpost(b["truth"][None], perstar=True)[1][0], b["cl"]) >= 0.8
    assert (np.asarray(b["cl"]["stage"]) == abi.STAGE_WD).sum() >= 4
    # a walker moves to a row of fewer common EEPs with steps to spare: where the GPU test cuts the block in two
    assert tags["shorter"] and tags["shorter"][0] < case.steps - 2


def test_the_cases_together_reach_every_tag():
    proposed = _sum(rw.CASES, "proposed")
    assert all(proposed[t] > 0 for t in rw.TAGS), [t for t in rw.TAGS if not proposed[t]]
    for cases in (rw.MARG_CASES, rw.GIVEN_CASES):
        accepted = _sum(cases, "accepted")
        for t in ("chunks_grew", "chunks_shrank", "cell_changed:age", "cell_changed:feh", "cell_changed:y", "one_interval", "valid_after_invalid"):
            assert accepted[t] >= 2, (t, accepted[t])
    accepted = _sum(rw.MARG_CASES, "accepted")
    assert accepted["run_eq_24"] > 0 and accepted["run_eq_25"] > 0 and accepted["run_gt_24"] > 0 and accepted["run_le_24"] > 0
    assert {c.n_filt for c in rw.MARG_CASES} == {c.n_filt for c in rw.GIVEN_CASES} == {3, 8, 12}
    assert {c.variant for c in rw.MARG_CASES} == {c.variant for c in rw.GIVEN_CASES} == set(rw.VARIANTS)


# ---- the comparator's power: one fault each -----------------------------------------------------------------------------------
class Honest:
    """the oracle itself, rebuilt from the case"""

    def __init__(self, case, b):
        self.case, self.b = case, b
        self.orc = oracle.Oracle(b["pack"], b["stars"], b["priors"], b["options"])

    def begin(self, start, lp0):
        pass

    def __call__(self, rows):
        return self.orc.logpost(rows)


class StaleOnInvalid(Honest):
    """a row without a log-posterior returns the walker's last one instead of -inf"""

    def begin(self, start, lp0):
        self.last = np.array(lp0)

    def __call__(self, rows):
        v = self.orc.logpost(rows)
        out = np.where(np.isfinite(v), v, self.last)
        self.last = out.copy()
        return out


class FirstEepIgnored(Honest):
    """the corner isochrones of a cell are read as if they all began at the cell's lowest first EEP"""

    def __call__(self, rows):
        out = np.empty(len(rows))
        for i, row in enumerate(rows):
            pack_d = dict(self.b["pack_d"])
            first = np.array(pack_d["iso_first_eep"])
            nA, nY = len(pack_d["log_age"]), len(pack_d["y"])
            for pop in range(self.case.n_pops):
                (ia, i_f, iy), _ = rw.cell_of(pack_d, row, pop)
                ks = [((i_f + df) * nY + iy + dy) * nA + ia + da for df in (0, 1) for dy in range(2 if nY > 1 else 1) for da in (0, 1)]
                first[ks] = first[ks].min()
            pack_d["iso_first_eep"] = first
            out[i] = oracle.Oracle(abi.make_pack(pack_d), self.b["stars"], self.b["priors"], self.b["options"]).logpost(row[None])[0]
        return out


class StaleLength(Honest):
    """a row whose common EEP range is shorter than that of the walker's row before it is evaluated on the longer range: the
    same pack, its isochrones padded at the upper end up to that length"""

    def _n(self, row):
        return max(rw.common_range(self.b["pack_d"], row, pop)[1] for pop in range(self.case.n_pops))

    def begin(self, start, lp0):
        self.prev = [self._n(r) for r in start]
        self.packs = {}

    def __call__(self, rows):
        out = np.array(self.orc.logpost(rows))
        for i, row in enumerate(rows):
            n = self._n(row)
            if np.isfinite(out[i]) and n < self.prev[i]:
                end = rw.common_range(self.b["pack_d"], row, 0)[2] + self.prev[i]
                if end not in self.packs:
                    c = self.case
                    self.packs[end] = abi.make_pack(rw.ladder_pack(c.n_filt, 3 if c.n_pops == 2 else 1, c.seed, c.variant, min_end=end))
                out[i] = oracle.Oracle(self.packs[end], self.b["stars"], self.b["priors"], self.b["options"]).logpost(row[None])[0]
            if np.isfinite(out[i]):
                self.prev[i] = n
        return out


def _first_fault(case, b, lp0, chain, log, stand_in):
    """The first step at which the stand-in, fed the proposals of the oracle's chain one step after the other, takes another
    decision than the oracle or records another log-posterior for an accepted move (beyond the comparator's 1e-10)."""
    from base_amd import mcmc
    stand_in.begin(b["start"], lp0)
    for s in range(case.steps):
        _, u = mcmc.draws(case.seed, s, b["ids"], len(b["free"]))
        cur = lp0 if s == 0 else chain[3][s - 1]
        v = stand_in(log.rows[s])
        with np.errstate(invalid="ignore"):
            took = (np.log(u) < v - cur) & np.isfinite(v)
            want = (np.log(u) < log.vals[s] - cur) & np.isfinite(log.vals[s])
        if np.any(took != want) or np.any(np.abs(v[want] - log.vals[s][want]) > 1e-10 * np.abs(log.vals[s][want])):
            return s
    return None


def _run(case, b, lp0, stand_in):
    stand_in.begin(b["start"], lp0)
    return rw.run_twin(case, b, stand_in, lp0)


@pytest.mark.parametrize("case", rw.CASES, ids=lambda c: c.name)
def test_the_oracle_passes_every_case(case):
    b, lp0, chain, log, _ = chain_of(case)
    rw.compare_chains(_run(case, b, lp0, Honest(case, b)), chain)


STAND_INS = [(StaleOnInvalid, "m-3f-1p-k2q2"), (StaleOnInvalid, "g-8f-2p"), (FirstEepIgnored, "m-8f-2p-k1q2"), (FirstEepIgnored, "g-3f-1p"),
             (StaleLength, "m-8f-1p-k3q2-wdragged"), (StaleLength, "g-12f-1p-flat")]


@pytest.mark.parametrize("stand_in,name", STAND_INS, ids=[f"{m.__name__}-{n}" for m, n in STAND_INS])
def test_a_faulty_stand_in_is_rejected_where_its_fault_first_matters(stand_in, name):
    case = next(c for c in rw.CASES if c.name == name)
    b, lp0, chain, log, _ = chain_of(case)
    want = _first_fault(case, b, lp0, chain, log, stand_in(case, b))
    assert want is not None, "the case never reaches the fault"
    with pytest.raises(rw.ChainMismatch) as e:
        rw.compare_chains(_run(case, b, lp0, stand_in(case, b)), chain)
    assert e.value.step == want, (e.value.step, want, str(e.value))
