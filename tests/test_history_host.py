"""The history checker's own power, on the CPU (tests/history_check.py; docs/LABNOTES.md section 15).

The runner and the deterministic sequences 1, 2, 5, 7 and the seeded random ones play here on a thin stand-in over the CPU
oracle, restricted to what the oracle states: logpost, sample_mass, derive_isochrone, sample_wd_mass.  The stand-in is rebuilt
from the configuration at every call, so used == fresh holds trivially and every sequence must pass.  Then five stand-ins
with ONE deliberately stale piece of state each: for each, a sequence must fail, and at the step where the stale state first
matters."""
import numpy as np
import pytest

import history_check as hc
import oracle
import wd_check
from base_amd import abi

GIVEN, MARG = hc.GIVEN, hc.MARG


@pytest.fixture(scope="module")
def world():
    return hc.World()


class OraclePlayer:
    """What a context would be if it kept no state but its configuration."""

    def __init__(self):
        self.cfg = None
        self.evaluated = False

    def close(self):
        pass

    def configure(self, op, args, cfg, world):
        self.cfg = cfg

    # -- what the evaluation uses (the mutants override these)
    def pack_for_stars(self):
        return self.cfg.pack

    def priors_key(self):
        return self.cfg.priors

    def grid(self):
        return self.cfg.options[2:]

    def _oracle(self, world, options=None):
        c = self.cfg
        return oracle.Oracle(world.pack(self.pack_for_stars())[1], world.stars(c.stars)[1], world.priors(self.priors_key()),
                             abi.make_options(*(options or c.options)))

    def evaluate(self, op, args, inp, cfg, world):
        out = self._evaluate(op, args, inp, world)
        self.evaluated = True
        return out

    def _evaluate(self, op, args, inp, world):
        rows, c = inp["rows"], self.cfg
        if op == "logpost":
            lp, ps = self._oracle(world).logpost(rows, perstar=True)
            return dict(logpost=lp, perstar=ps) if args[1] else dict(logpost=lp)
        if op == "sample_mass":
            K, Q = self.grid()
            m, q, mem, pop, _ = self._oracle(world, c.options[:2] + (K, Q)).sample_mass(rows, seed=inp["seed"], row0=7 * inp["index"])
            return dict(mass=m, ratio=q, member=mem, pop=pop)
        if op == "derive_isochrone":
            first, mass, mags, tip = oracle.derive_isochrone(oracle.load(), world.pack(c.pack)[1], rows[0], int(args[0]))
            return dict(first_eep=np.int32(first), mass=mass, mags=mags, agb_tip=np.float64(tip))
        if op == "sample_wd_mass":
            # not the draw itself (the oracle has none): each WD-stage star's catalogue mass moved to the nearest of n_nodes equal
            # steps between the AGB tip and the pack's upper WD mass, and the WD chain's quantities there (wd_check) -- a function
            # of the pack, the stars, the row and n_nodes, which is all the history check needs of it
            pack_d = world.pack(self.pack_for_stars())[0]
            cl = world.stars(c.stars)[0]
            wd = np.flatnonzero(np.asarray(cl["stage"]) == abi.STAGE_WD)
            res = {k: np.zeros((rows.shape[0], wd.size)) for k in ("zams", "wd_mass", "prec_log_age", "log_cool_age", "log_teff", "logg")}
            for r, row in enumerate(rows):
                iso = oracle.derive_isochrone(oracle.load(), world.pack(self.pack_for_stars())[1], row, 0)
                if wd.size == 0 or iso[1].size == 0:
                    continue
                tip, top, n = iso[3], float(pack_d["m_wd_up"]), int(args[1])
                j = np.clip(np.rint((np.asarray(cl["mass1"])[wd] - tip) / (top - tip) * n), 1, n)
                z = tip + (top - tip) * j / n
                vals = wd_check.wd_chain(pack_d, row, z)
                res["zams"][r] = z
                for k, v in zip(("wd_mass", "prec_log_age", "log_cool_age", "log_teff", "logg"), vals):
                    res[k][r] = v
            return res
        raise KeyError(op)


# ---- the mutants: one stale piece of state each ---------------------------------------------------------------------------
class IgnoresPriorsOnceEvaluated(OraclePlayer):
    stale = None

    def configure(self, op, args, cfg, world):
        if op == "set_priors" and self.evaluated:
            self.stale = self.priors_key()
        self.cfg = cfg

    def priors_key(self):
        return self.stale or self.cfg.priors


class KeepsFirstGrid(OraclePlayer):
    """sample_mass with the (K, Q) of the first b9_set_options"""
    first = None

    def configure(self, op, args, cfg, world):
        self.cfg = cfg
        if op == "set_options" and self.first is None:
            self.first = cfg.options[2:]

    def grid(self):
        return self.first or self.cfg.options[2:]


class RestagesOnLoadStarsOnly(OraclePlayer):
    """the stars stay staged against the pack in force at b9_load_stars"""
    staged = None

    def configure(self, op, args, cfg, world):
        self.cfg = cfg
        if op == "load_stars":
            self.staged = cfg.pack

    def pack_for_stars(self):
        return self.staged or self.cfg.pack


class LargestCatalogueTruncated(OraclePlayer):
    """per-star arrays of the largest catalogue seen, truncated to the current one's length"""
    largest = None

    def configure(self, op, args, cfg, world):
        self.cfg = cfg
        if op == "load_stars" and (self.largest is None or world.catalogues[cfg.stars[1]][0] >= world.catalogues[self.largest.stars[1]][0]):
            self.largest = cfg

    def _evaluate(self, op, args, inp, world):
        out = super()._evaluate(op, args, inp, world)
        if op == "logpost" and args[1] and self.largest is not None and self.largest.stars != self.cfg.stars:
            big = self.cfg.copy()
            big.stars = self.largest.stars
            now, self.cfg = self.cfg, big
            try:
                out["perstar"] = super()._evaluate(op, args, inp, world)["perstar"][:, :out["perstar"].shape[1]].copy()
            finally:
                self.cfg = now
        return out


class StalePartial(OraclePlayer):
    """the previous call's last per-star value added into this call's first"""
    carry = 0.0

    def _evaluate(self, op, args, inp, world):
        out = super()._evaluate(op, args, inp, world)
        if op == "logpost" and args[1]:
            out["perstar"] = out["perstar"].copy()
            last = float(out["perstar"][-1, -1])
            out["perstar"][0, 0] += self.carry
            self.carry = last if np.isfinite(last) else 0.0
        return out


# ---- the honest stand-in passes every sequence --------------------------------------------------------------------------------
def seq_priors_host():
    """sequence 7 on the catalogue of 300 (the oracle's brute-force integral over 2500 stars would dominate the CPU suite)"""
    return [(st[0], "c300") if st[0] == "load_stars" else st for st in hc.seq_priors()]


SEQUENCES = {
    "1": hc.seq_isochrone_length, "2": hc.seq_filter_width, "5": hc.seq_modes_and_grids, "7": seq_priors_host,
    **{f"8/{s}": (lambda s=s: hc.random_sequence(s, 14)) for s in (11, 12, 13, 14, 15, 16)},
}


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_the_stateless_stand_in_passes(world, name):
    steps = hc.host_subset(SEQUENCES[name]())
    r = hc.play(name, steps, world, OraclePlayer)
    assert r["compared"] == sum(st[0] in hc.EVAL_OPS for st in steps) > 0


def _index(steps, pred):
    """index of the first evaluating step for which pred(step, configuration steps before it, evaluating steps before it) holds"""
    conf, evals = [], []
    for i, st in enumerate(steps):
        if st[0] in hc.CONFIG_OPS:
            conf.append(st)
            continue
        if pred(st, conf, evals):
            return i
        evals.append(st)
    raise AssertionError("the sequence never reaches the stale state")


def _perstar(st):
    return st[0] == "logpost" and st[1 + 1]


def _uses_stars(st):
    return st[0] in ("logpost", "sample_mass", "sample_wd_mass")


def _priors_changed_after_an_evaluation(st, conf, evals):
    # a logpost after a set_priors of ANOTHER name that followed an evaluation (sequence 7 opens with "default" twice)
    names = [c[1] for c in conf if c[0] == "set_priors"]
    return st[0] == "logpost" and bool(evals) and len(set(names)) > 1


def _second_grid(st, conf, evals):
    grids = [c[3:] for c in conf if c[0] == "set_options"]
    return st[0] == "sample_mass" and grids[-1] != grids[0]


def _pack_reloaded_alone(st, conf, evals):
    return _uses_stars(st) and conf[-1][0] == "load_pack"


def _smaller_catalogue(st, conf, evals):
    cats = [c[1] for c in conf if c[0] == "load_stars"]
    return _perstar(st) and len(cats) > 1 and hc.CATALOGUES[cats[-1]][0] < max(hc.CATALOGUES[c][0] for c in cats[:-1])


def _second_perstar(st, conf, evals):
    return _perstar(st) and any(_perstar(e) for e in evals)


MUTANTS = [
    (IgnoresPriorsOnceEvaluated, "7", _priors_changed_after_an_evaluation, "logpost"),
    (KeepsFirstGrid, "5", _second_grid, None),
    (RestagesOnLoadStarsOnly, "2", _pack_reloaded_alone, None),
    (LargestCatalogueTruncated, "1", _smaller_catalogue, "perstar"),
    (StalePartial, "1", _second_perstar, "perstar"),
]


@pytest.mark.parametrize("mutant,name,pred,output", MUTANTS, ids=[m[0].__name__ for m in MUTANTS])
def test_a_stale_stand_in_is_caught_where_its_state_first_matters(world, mutant, name, pred, output):
    steps = hc.host_subset(SEQUENCES[name]())
    want = _index(steps, pred)
    with pytest.raises(hc.HistoryMismatch) as e:
        hc.play(name, steps, world, lambda: OraclePlayer(), used=mutant())
    assert e.value.step_index == want, (e.value.step_index, want, str(e.value))
    if output:
        assert e.value.output == output
    assert repr(steps[want]) in str(e.value) and "history:" in str(e.value)


def test_comparator_counts_nan_inf_and_signed_zero():
    a = np.array([1.0, np.nan, -np.inf, 0.0])
    assert hc.first_difference(a, a.copy()) is None
    assert hc.first_difference(a, np.array([1.0, np.nan, -np.inf, -0.0]))[0] == (3,)
    assert hc.first_difference(a, np.array([1.0, 0.0, -np.inf, 0.0]))[0] == (1,)
    assert hc.first_difference(a, a[:3])[0] == "shape"
    assert hc.first_difference(np.int64(3), np.int64(4)) == ((), 3, 4)
    assert hc.compare_outputs(dict(x=a, n=np.int64(1)), dict(x=a.copy(), n=np.int64(2)))[0] == "n"


def test_random_sequences_are_legal_and_reproducible():
    for seed in (11, 12, 13, 14, 15, 16):
        s = hc.random_sequence(seed, 14)
        assert s == hc.random_sequence(seed, 14)
        cfg = hc.Config()
        for st in s:
            if st[0] in hc.CONFIG_OPS:
                cfg = cfg.apply(st[0], st[1:])
                continue
            assert st[0] in hc.EVAL_OPS
            # complete, and the stars and priors belong to a pack of the loaded one's filter count
            assert cfg.pack and cfg.stars and cfg.priors
            assert hc.PACKS[cfg.stars[0]]["n_filt"] == hc.PACKS[cfg.pack]["n_filt"]
        assert sum(st[0] in hc.EVAL_OPS for st in s) >= 4
