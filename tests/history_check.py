"""History independence of a context: a small language of call sequences, a runner and a bitwise comparator.

The property (docs/LABNOTES.md section 15): for any sequence of ABI calls on one context, the outputs of every call are bit
for bit the outputs of the same call on a fresh context brought directly to the used context's CURRENT configuration
(pack, stars, priors, options, tuning).  No GPU dependence here: the runner plays a sequence on any "player" -- the GPU engine
(GpuPlayer, tests/test_gpu_history.py), a stand-in over the CPU oracle or one of its deliberately stale mutants
(tests/test_history_host.py).

A step is a tuple (operation, *arguments).
  configuration:  ("load_pack", name)  ("load_stars", name)  ("set_priors", name)  ("set_options", mode, n_pops, K, Q)
                  ("set_tuning", {field: value})
  evaluating:     ("logpost", W, perstar)  ("logpost_device", W)  ("block", W, n_steps, record, rows)
                  ("block_pipelined", W, sizes)  ("sample_mass", n_rows)  ("sample_wd_mass", n_rows, n_nodes)
                  ("derive_isochrone", pop)  ("predict_mags", n)
  an evaluating step may end in "off": its last parameter row then lies outside the grid (log age beyond the pack's axis).
The inputs of an evaluating step (parameter rows, start states, proposal factor, seeds, masses) are functions of the current
configuration and the step's index only, so the used and the fresh player get identical bytes.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

from base_amd import abi, mcmc, synth

CONFIG_OPS = ("load_pack", "load_stars", "set_priors", "set_options", "set_tuning")
EVAL_OPS = ("logpost", "logpost_device", "block", "block_pipelined", "sample_mass", "sample_wd_mass", "derive_isochrone", "predict_mags")
GIVEN, MARG = abi.MODE_GIVEN_MASS, abi.MODE_MARGINALISED

# ---- the named packs and catalogues ---------------------------------------------------------------------------------------
# (n_y = 3 everywhere but L: a second population then has an isochrone of its own)
PACKS = {
    "G3": dict(name="girardi", n_filt=3, n_y=3, n_feh=4, n_age=8, n_eep=90),                  # padded width 4
    "P8": dict(name="parsec", n_filt=8, n_y=3, n_feh=4, n_age=8, n_eep=90),
    "P8b": dict(name="parsec", n_filt=8, n_y=3, n_feh=4, n_age=8, n_eep=90, ifmr_id=abi.IFMR_SALARIS_LIN, m_wd_up=7.0),   # same filter names
    "P16": dict(name="parsec", n_filt=16, n_y=3, n_feh=4, n_age=8, n_eep=90),
    "D5": dict(name="dsed", n_filt=5, n_y=3, n_feh=4, n_age=8, n_eep=90, wd_ragged=True),     # 3 helium nodes, ragged cooling tracks
    "L": dict(name="parsec", n_filt=8, n_y=1, n_feh=3, n_age=4, n_eep=2000),                  # test_long_isochrone_2000_eeps' pack
}
CATALOGUES = {          # name -> (stars, WD-stage fraction)
    "one": (1, 0.0), "c65": (65, 0.0), "c300": (300, 0.10), "wd1300": (1300, 0.5), "c2500": (2500, 0.08),
}


class World:
    """The named packs, catalogues and priors, made once per test module and never changed."""

    def __init__(self, extra_catalogues: Optional[Dict[str, Tuple[int, float]]] = None):
        self._packs, self._stars = {}, {}
        self.catalogues = dict(CATALOGUES)
        self.catalogues.update(extra_catalogues or {})

    def pack(self, name):
        if name not in self._packs:
            kw = dict(PACKS[name])
            m_wd_up = kw.pop("m_wd_up", None)
            d = synth.make_pack(kw.pop("name"), **kw)
            if m_wd_up:
                d["m_wd_up"] = m_wd_up
            self._packs[name] = (d, abi.make_pack(d))
        return self._packs[name]

    def truth(self, pack_name):
        return synth.default_params(self.pack(pack_name)[0])

    def stars(self, key):
        """key = (pack the catalogue was drawn for, catalogue name)"""
        if key not in self._stars:
            pack_name, name = key
            n, wd_frac = self.catalogues[name]
            seed = 9000 + sum(map(ord, pack_name + name))
            cl = synth.make_cluster(self.pack(pack_name)[0], n, seed=seed, truth=self.truth(pack_name), wd_frac=wd_frac)
            self._stars[key] = (cl, abi.make_stars(cl))
        return self._stars[key]

    def bad_stars(self, key):
        """the catalogue with one non-finite observation in a filter in use: b9_load_stars must refuse it"""
        cl = dict(self.stars(key)[0])
        obs = np.array(cl["obs"], dtype=np.float64)
        sig = np.asarray(cl["sigma"]).reshape(obs.shape)
        i = int(np.flatnonzero(sig[:, 0] > 0)[0])
        obs[i, 0] = np.inf
        cl["obs"] = obs
        return abi.make_stars(cl)

    def priors(self, key):
        """key = (pack the priors were made for, name)"""
        pack_name, name = key
        pack_d = self.pack(pack_name)[0]
        truth = self.truth(pack_name)
        pr = synth.default_priors(pack_d, truth, 2)
        ages, fehs = np.asarray(pack_d["log_age"]), np.asarray(pack_d["feh"])
        if name == "default":
            pass
        elif name == "moved":          # the means one cell further in log age and [Fe/H]: the marginalised plan's reference row moves
            ia = int(np.searchsorted(ages, truth[abi.P_LOGAGE], side="right")) - 1
            i_f = int(np.searchsorted(fehs, truth[abi.P_FEH], side="right")) - 1
            step_a = ages[ia + 1] - ages[ia] if ia + 2 < len(ages) else -(ages[ia] - ages[ia - 1])
            step_f = fehs[i_f + 1] - fehs[i_f] if i_f + 2 < len(fehs) else -(fehs[i_f] - fehs[i_f - 1])
            pr.mean[abi.P_LOGAGE] = truth[abi.P_LOGAGE] + step_a
            pr.mean[abi.P_FEH] = truth[abi.P_FEH] + step_f
        elif name == "narrow":         # a log-age window that ends below every evaluated row (rows scatter 0.0006 about the truth)
            pr.log_age_max = truth[abi.P_LOGAGE] - 0.05
        elif name == "nan":            # no usable reference row
            pr.mean[abi.P_LOGAGE] = float("nan")
            pr.mean[abi.P_FEH] = float("nan")
        else:
            raise KeyError(name)
        return pr


class Config:
    """What a context is configured with, by name.  Stars and priors remember the pack in force when they were set."""

    def __init__(self):
        self.pack = None
        self.stars = None          # (pack name, catalogue name)
        self.priors = None         # (pack name, priors name)
        self.options = (GIVEN, 1, 8, 8)
        self.tuning: Dict[str, int] = {}
        self.history: List[Tuple] = []

    def copy(self):
        c = Config()
        c.pack, c.stars, c.priors, c.options, c.tuning, c.history = self.pack, self.stars, self.priors, self.options, dict(self.tuning), list(self.history)
        return c

    def apply(self, op, args):
        c = self.copy()
        if op == "load_pack":
            c.pack = args[0]
        elif op == "load_stars":
            c.stars = (self.pack, args[0])
        elif op == "set_priors":
            c.priors = (self.pack, args[0])
        elif op == "set_options":
            c.options = tuple(int(a) for a in args)
        elif op == "set_tuning":
            c.tuning = dict(args[0]) if args else {}
        else:
            raise KeyError(op)
        c.history.append((op,) + tuple(args))
        return c

    def steps(self):
        """the configuration as the steps that bring a fresh context to it, in the order of the ABI's documentation"""
        s = [("load_pack", self.pack), ("load_stars",) + self.stars, ("set_priors",) + self.priors, ("set_options",) + self.options,
             ("set_tuning", dict(self.tuning))]
        return s

    def n_filt(self, world):
        return world.pack(self.pack)[0]["n_filt"]

    def __repr__(self):
        return f"pack={self.pack} stars={self.stars} priors={self.priors} options={self.options} tuning={self.tuning}"


def is_off(args):
    return bool(args) and args[-1] == "off"


def free_and_chol(n_pops):
    free = list(mcmc.DEFAULT_FREE) + ([abi.P_Y, abi.P_Y2, abi.P_LAMBDA] if n_pops == 2 else [])
    chol = np.diag([3e-4, 2e-3, 8e-4, 6e-4] + ([3e-4, 3e-4, 2e-3] if n_pops == 2 else []))
    return np.array(free, dtype=np.int32), chol


def make_inputs(op, args, cfg: Config, index: int, world: World) -> Dict:
    """The inputs of evaluating step `index`: a function of the configuration and the index only."""
    pack_d = world.pack(cfg.pack)[0]
    truth = world.truth(cfg.pack)
    n_pops = cfg.options[1]
    n_rows = 1 if op in ("derive_isochrone", "predict_mags") else args[0]
    rows = synth.walker_params(truth, int(n_rows), seed=index, scale=0.03, n_pops=n_pops)
    if is_off(args):
        rows[-1, abi.P_LOGAGE] = float(pack_d["log_age"][-1]) + 0.5
    inp = dict(rows=rows, seed=1000 + index, index=index)
    if op in ("block", "block_pipelined"):
        inp["free"], inp["chol"] = free_and_chol(n_pops)
        inp["ids"] = np.arange(int(n_rows), dtype=np.int32) + 3 * index
        inp["step0"] = 1000 * index
    if op == "predict_mags":
        rng = np.random.default_rng(index)
        n = int(args[0])
        inp["mass1"] = rng.uniform(0.2, 7.5, n)
        inp["mass_ratio"] = np.where(rng.random(n) < 0.4, rng.uniform(0.0, 1.0, n), 0.0)
        inp["wd_type"] = (rng.random(n) < 0.3).astype(np.int32)
        inp["pop"] = (rng.random(n) < 0.5).astype(np.int32)
    return inp


# ---- the comparator -------------------------------------------------------------------------------------------------------
class HistoryMismatch(AssertionError):
    def __init__(self, sequence, step_index, step, output, where, used, fresh, cfg: Config):
        self.sequence, self.step_index, self.step, self.output, self.where = sequence, step_index, step, output, where
        super().__init__(f"sequence {sequence!r}, step {step_index} {step!r}: output {output!r} differs at index {where}: used context {used!r}, "
                         f"fresh context {fresh!r}\n  configuration: {cfg!r}\n  history: " + " ; ".join(map(repr, cfg.history)))


def _bits(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
    return a


def first_difference(a, b):
    """None when a and b are the same bits (NaN and -inf patterns and the sign of zero count), else (index, a there, b there)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return ("shape", (a.shape, str(a.dtype)), (b.shape, str(b.dtype)))
    ne = np.flatnonzero(_bits(a).ravel() != _bits(b).ravel())
    if ne.size == 0:
        return None
    i = int(ne[0])
    return (tuple(int(k) for k in np.unravel_index(i, a.shape)) if a.ndim else (), a.ravel()[i].item(), b.ravel()[i].item())


def compare_outputs(got: Dict, want: Dict):
    """(output name, index, used, fresh) of the first difference between two evaluating steps' outputs, or None."""
    if list(got) != list(want):
        return ("<names>", (), list(got), list(want))
    for k in got:
        d = first_difference(got[k], want[k])
        if d is not None:
            return (k,) + d
    return None


# ---- the runner -----------------------------------------------------------------------------------------------------------
def bring_to(player, cfg: Config, world: World):
    for st in cfg.steps():
        player.configure(st[0], st[1:], cfg, world)
    return player


def play(name: str, steps, world: World, make_player: Callable, witness: Optional[Callable] = None, used=None,
         prepare: Optional[Callable] = None, on_step: Optional[Callable] = None) -> Dict:
    """Play `steps` on one long-lived player; after every evaluating step play that step alone on a fresh player from
    make_player() brought to the current configuration and compare every output bit for bit (HistoryMismatch on the first
    difference).  witness(op, args, inputs, outputs, cfg), when given, is called for the LAST evaluating step: the fresh context
    is the same code, so an independent statement has the last word.  prepare(op, args, inputs, cfg) may add to a step's inputs
    what neither player under comparison should compute for itself (a block's starting log-posteriors: taking them from the
    player would make b9_logpost, not the block, the first call after a reconfiguration); on_step(index, step, outputs, cfg)
    sees every compared step's outputs.  Returns {"compared": evaluating steps compared}."""
    own = used is None
    used = used or make_player()
    cfg = Config()
    last_eval = max((i for i, st in enumerate(steps) if st[0] in EVAL_OPS), default=-1)
    compared = 0
    try:
        for i, st in enumerate(steps):
            op, args = st[0], tuple(st[1:])
            if op in CONFIG_OPS:
                cfg = cfg.apply(op, args)
                used.configure(op, args, cfg, world)
                continue
            if op not in EVAL_OPS:
                raise KeyError(op)
            inputs = make_inputs(op, args, cfg, i, world)
            if prepare is not None:
                prepare(op, args, inputs, cfg)
            got = used.evaluate(op, args, inputs, cfg, world)
            fresh = make_player()
            try:
                want = bring_to(fresh, cfg, world).evaluate(op, args, inputs, cfg, world)
            finally:
                fresh.close()
            d = compare_outputs(got, want)
            if d is not None:
                raise HistoryMismatch(name, i, st, d[0], d[1], d[2], d[3], cfg)
            compared += 1
            if on_step is not None:
                on_step(i, st, got, cfg)
            if witness is not None and i == last_eval:
                witness(op, args, inputs, got, cfg)
    finally:
        if own:
            used.close()
    return dict(compared=compared)


# ---- seeded random sequences ----------------------------------------------------------------------------------------------
RANDOM_PACKS, RANDOM_CATALOGUES = ("G3", "P8", "D5"), ("one", "c65", "c300")


def random_sequence(seed: int, n_steps: int = 14):
    """A legal sequence of n_steps steps after the opening configuration, drawn from the whole alphabet with a plain numpy
    generator: the stars follow a pack of another filter count at once (and the priors, whose log-age window is the pack's),
    evaluating steps only run on a complete configuration."""
    rng = np.random.default_rng(seed)
    pick = lambda xs: xs[int(rng.integers(len(xs)))]          # noqa: E731
    pack = pick(RANDOM_PACKS)
    steps = [("load_pack", pack), ("load_stars", pick(RANDOM_CATALOGUES)), ("set_priors", "default"), ("set_options", GIVEN, 1, 2, 2)]
    mode, off_used = GIVEN, False
    grids = ((1, 2), (2, 2), (3, 1), (2, 3))
    n = 0
    while n < n_steps:
        r = rng.random()
        if r < 0.10:
            pack = pick(RANDOM_PACKS)
            steps += [("load_pack", pack), ("load_stars", pick(RANDOM_CATALOGUES)), ("set_priors", "default")]
        elif r < 0.20:
            steps.append(("load_stars", pick(RANDOM_CATALOGUES)))
        elif r < 0.25:
            steps.append(("set_priors", pick(("default", "moved", "nan"))))
        elif r < 0.37:
            mode = pick((GIVEN, MARG))
            steps.append(("set_options", mode, int(rng.integers(1, 3))) + pick(grids))
        elif r < 0.45:
            steps.append(("set_tuning", pick(({}, {"tree_depth": 1}, {"tree_depth": 2}, {"tree_depth": 3}, {"heavy_parts": 9}, {"two_launch_steps": 1},
                                              {"tiles_per_block": 2}, {"marg_piece_units": 2}))))
        else:
            op = pick(EVAL_OPS)
            W = int(pick((1, 2, 3, 8)))
            st = {"logpost": ("logpost", W, bool(rng.random() < 0.5)), "logpost_device": ("logpost_device", W),
                  "block": ("block", min(W, 4), int(rng.integers(20, 31)), bool(rng.random() < 0.7), bool(rng.random() < 0.5)),
                  "block_pipelined": ("block_pipelined", min(W, 4), (7, 20, 1, 13)), "sample_mass": ("sample_mass", int(rng.integers(1, 4))),
                  "sample_wd_mass": ("sample_wd_mass", 2, int(pick((1, 16, 65)))), "derive_isochrone": ("derive_isochrone", int(rng.integers(0, 2))),
                  "predict_mags": ("predict_mags", int(pick((1, 200))))}[op]
            if not off_used and op in ("logpost", "sample_mass", "sample_wd_mass", "derive_isochrone", "predict_mags") and rng.random() < 0.3:
                st, off_used = st + ("off",), True
            steps.append(st)
        n += 1
    return steps + [("logpost", 2, True)]


# ---- the GPU player -------------------------------------------------------------------------------------------------------
class GpuPlayer:
    """One b9_ctx behind base_amd.engine.Engine."""

    def __init__(self, lib=None):
        from base_amd import engine
        self.eng = engine.Engine(lib=lib)
        self._hip = None

    def close(self):
        self.eng.close()

    def configure(self, op, args, cfg: Config, world: World):
        e = self.eng
        if op == "load_pack":
            e.load_pack(world.pack(cfg.pack)[1])
        elif op == "load_stars":
            e.load_stars(world.stars(cfg.stars)[1])
        elif op == "set_priors":
            e.set_priors(world.priors(cfg.priors))
        elif op == "set_options":
            e.set_options(abi.make_options(*cfg.options))
        elif op == "set_tuning":
            e.set_tuning(**cfg.tuning)

    # -- device memory for b9_logpost_device, through the HIP runtime the library already loaded (torch tensors, as
    #    tests/test_gpu_edges.py uses them, need a child process: torch must initialise its own runtime before the library loads)
    def _device_logpost(self, rows, n_stars):
        if self._hip is None:
            self._hip = C.CDLL("libamdhip64.so")
            self._hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            self._hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            self._hip.hipFree.argtypes = [C.c_void_p]
        hip, W = self._hip, rows.shape[0]
        lp, ps = np.full(W, 123.0), np.full((W, n_stars), 123.0)
        bufs = []

        def dev(nbytes):
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), nbytes) == 0
            bufs.append(p)
            return p
        try:
            d_par, d_lp, d_ps = dev(rows.nbytes), dev(lp.nbytes), dev(ps.nbytes)
            assert hip.hipMemcpy(d_par, rows.ctypes.data, rows.nbytes, 1) == 0
            self.eng.logpost_device(d_par.value, W, d_lp.value, d_ps.value)
            assert hip.hipDeviceSynchronize() == 0
            assert hip.hipMemcpy(lp.ctypes.data, d_lp, lp.nbytes, 2) == 0
            assert hip.hipMemcpy(ps.ctypes.data, d_ps, ps.nbytes, 2) == 0
        finally:
            for p in bufs:
                hip.hipFree(p)
        return lp, ps

    def evaluate(self, op, args, inp, cfg: Config, world: World) -> Dict:
        e, rows = self.eng, inp["rows"]
        if op == "logpost":
            if args[1]:
                lp, ps = e.logpost(rows, perstar=True)
                return dict(logpost=lp, perstar=ps)
            return dict(logpost=e.logpost(rows))
        if op == "logpost_device":
            lp, ps = self._device_logpost(np.ascontiguousarray(rows), e.n_stars)
            return dict(logpost=lp, perstar=ps)
        if op == "block":
            W, n_steps, record, want_rows = args[:4]
            lp0 = inp["lp0"]            # (from a helper context: the block is this context's first call after a reconfiguration)
            origin = rows[:, inp["free"]].mean(axis=0) if want_rows else None
            h = e.mcmc_submit(rows, lp0, inp["ids"], inp["free"], inp["chol"], inp["seed"], inp["step0"], n_steps, record=record,
                              asynchronous=False, row_origin=origin)
            p, l, x, y, a = e.mcmc_collect(h)
            out = dict(lp0=lp0, params=p, logpost=l, n_accept=np.int64(a))
            if record:
                out.update(samples=x, lps=y)
            if want_rows:
                out["rows"] = h["rows"]
            return out
        if op == "block_pipelined":
            sizes = args[1]
            lp0 = inp["lp0"]
            origin = rows[:, inp["free"]].mean(axis=0)
            handles, done, step0 = [], [], inp["step0"]
            for k, s in enumerate(sizes):          # CONTINUE | ASYNC, at most two outstanding, collected in order
                if len(handles) == 2:
                    done.append((handles[0], e.mcmc_collect(handles.pop(0))))
                handles.append(e.mcmc_submit(rows, lp0, inp["ids"], inp["free"], inp["chol"], inp["seed"], step0, s, record=True, cont=k > 0,
                                             asynchronous=True, row_origin=origin))
                step0 += s
            while handles:
                done.append((handles[0], e.mcmc_collect(handles.pop(0))))
            out = dict(lp0=lp0, params=done[-1][1][0], logpost=done[-1][1][1], samples=np.concatenate([r[2] for _, r in done]),
                       lps=np.concatenate([r[3] for _, r in done]), n_accept=np.array([r[4] for _, r in done], dtype=np.int64))
            for k, (h, _) in enumerate(done):
                out[f"rows{k}"] = h["rows"]
            return out
        if op == "sample_mass":
            m, q, mem, pop = e.sample_mass(rows, seed=inp["seed"], row0=7 * inp["index"])
            return dict(mass=m, ratio=q, member=mem, pop=pop)
        if op == "sample_wd_mass":
            return e.sample_wd_mass(rows, int(args[1]), seed=inp["seed"], row0=7 * inp["index"])
        if op == "derive_isochrone":
            first, mass, mags, tip = e.derive_isochrone(rows[0], int(args[0]))
            return dict(first_eep=np.int32(first), mass=mass, mags=mags, agb_tip=np.float64(tip))
        if op == "predict_mags":
            pop = inp["pop"] if cfg.options[1] == 2 else None
            mags, stage = e.predict_mags(rows[0], inp["mass1"], inp["mass_ratio"], inp["wd_type"], pop)
            return dict(mags=mags, stage=stage)
        raise KeyError(op)


# ---- the deterministic sequences (docs/LABNOTES.md section 15 numbers them) --------------------------------------------------
def conf(pack, stars, priors="default"):
    return [("load_pack", pack), ("load_stars", stars), ("set_priors", priors)]


def _battery(off=False):
    """the evaluating steps sequences 1 and 2 run at every pack: both logpost forms, a block of one walker (the tree launch
    where the automatic plan takes it) and of eight (the one-step launch), the isochrone, the forward model, the WD draws"""
    return [("logpost", 8, True), ("logpost", 1, False) + (("off",) if off else ()), ("block", 1, 24, True, True), ("block", 8, 20, True, False),
            ("derive_isochrone", 0), ("predict_mags", 200), ("sample_wd_mass", 2, 65)]


def seq_isochrone_length():
    """1. L -> P8 -> L -> P8, given-mass: mass_cap, iso_stride and every buffer behind them grow and shrink; the smaller
    catalogue follows the larger one (perstar_cap keeps the larger's tail)."""
    s = [("set_options", GIVEN, 1, 2, 2)]
    for k, p in enumerate(("L", "P8", "L", "P8")):
        s += conf(p, "c300" if p == "L" else "c65") + _battery(off=k == 1)
    return s + [("logpost", 2, True)]


def seq_filter_width():
    """2. G3 -> P8 -> (P8b: the pack alone, same filter names -- the stars are restaged through stars_dirty) -> P16 -> G3, c300
    reloaded for each."""
    s = [("set_options", GIVEN, 1, 2, 2)]
    for k, p in enumerate(("G3", "P8", "P16", "G3")):
        s += conf(p, "c300") + _battery(off=k == 2)
        if p == "P8":
            s += [("load_pack", "P8b"), ("logpost", 2, True), ("block", 2, 20, True, True), ("sample_wd_mass", 2, 65)]
    return s + [("logpost", 2, True)]


def seq_walker_counts():
    """3. one configuration, W = 8, 1, 3, 1, 8, 2: cap_walkers grows once and every later call lives inside the larger buffers."""
    pipe = (7, 20, 1, 13)
    return [("set_options", GIVEN, 1, 2, 2)] + conf("P8", "c300") + [
        ("logpost", 8, True), ("block", 1, 24, True, True), ("block_pipelined", 3, pipe), ("logpost", 1, False, "off"), ("block", 8, 20, True, False),
        ("block_pipelined", 2, pipe), ("logpost", 8, False), ("block_pipelined", 1, pipe), ("logpost", 3, True), ("block", 2, 24, True, True)]


def seq_heavy_share(n_pops):
    """4. wd1300 -> c65 -> wd1300 -> one, then on c300 heavy_parts = 9, automatic, tree_depth = 1, 2, 3, 0: the tree partials'
    inner stride (n_groups * 4 + heavy_parts + 1) & ~1 changes inside an unchanged capacity; n_pops changes the lane layout
    and heavy_parts.  After each: a block of one walker and a block of four."""
    blocks = [("block", 1, 21, True, True), ("block", 4, 20, True, False)]
    s = [("set_options", GIVEN, n_pops, 2, 2), ("load_pack", "P8")]
    for k, c in enumerate(("wd1300", "c65", "wd1300", "one")):
        s += [("load_stars", c)] + ([("set_priors", "default")] if k == 0 else []) + blocks
    s[-1] += ("off",)              # (the fourth walker starts outside the grid and never finds a way back)
    s += [("load_stars", "c300")]
    for t in ({"heavy_parts": 9}, {}, {"tree_depth": 1}, {"tree_depth": 2}, {"tree_depth": 3}, {"tree_depth": 0}):
        s += [("set_tuning", t)] + blocks
    return s


def seq_modes_and_grids():
    """5. c300: given-mass; marginalised (3, 3), (1, 8), (4, 2); given-mass; two populations given-mass, marginalised (2, 2); one
    population.  At each: logpost, a block in the mode's own form and with two_launch_steps, sample_mass (the marginalised grid
    whatever the mode), sample_wd_mass at 8 K and 1000 nodes."""
    s = conf("P8", "c300")
    for o in ((GIVEN, 1, 2, 2), (MARG, 1, 3, 3), (MARG, 1, 1, 8), (MARG, 1, 4, 2), (GIVEN, 1, 4, 2), (GIVEN, 2, 4, 2), (MARG, 2, 2, 2), (MARG, 1, 2, 2)):
        s += [("set_options",) + o, ("logpost", 2, True), ("block", 2, 20, True, True), ("set_tuning", {"two_launch_steps": 1}), ("block", 2, 20, True, True),
              ("set_tuning", {}), ("sample_mass", 3), ("sample_wd_mass", 2, 8 * o[2]), ("sample_wd_mass", 2, 1000)]
    s[-3] = ("sample_mass", 3, "off")
    return s + [("logpost", 2, True)]


def seq_split_unsplit():
    """6. marginalised (2, 2): c2500 (split into pieces; marg_piece_units 2, 9, 0 -- each against a fresh context AT that setting)
    -> big (one star above the unsplit threshold) -> c2500 -> c65: the shares, the plan's allocations, the never-shrunk tables."""
    s = [("set_options", MARG, 1, 2, 2)] + conf("G3", "c2500") + [("logpost", 2, True)]
    for u in (2, 9, 0):
        s += [("set_tuning", {"marg_piece_units": u}), ("logpost", 2, True)]
    s += [("load_stars", "big"), ("logpost", 2, True), ("load_stars", "c2500"), ("logpost", 2, True, "off"), ("load_stars", "c65"), ("logpost", 2, True)]
    return s


def seq_priors():
    """7. marginalised (3, 3) on c2500: the plan's reference row moves by a cell, the window excludes the rows (-inf), NaN means
    (no usable reference), the original priors; logpost and a 20-step block after each."""
    s = [("set_options", MARG, 1, 3, 3)] + conf("P8", "c2500")
    for p in ("default", "moved", "narrow", "nan", "default"):
        s += [("set_priors", p), ("logpost", 1, True), ("block", 2, 20, True, False) + (("off",) if p == "moved" else ())]
    return s + [("logpost", 1, True)]


def seq_first_call():
    """11. (added to the issue's list) The canonical tile groups key on mass_cap through the occupancy query, and mass_cap
    follows the loaded pack only once the work buffers are sized.  The long pack comes first, so that the used context's stale
    value is the LARGE one (2000 EEPs: a mass column of 16 KB in LDS, fewer resident workgroups) when the short pack arrives
    with a catalogue of 79 tiles; the fresh context's is 0.  A given-mass two-launch block (its launch_stars takes the plan
    b9_mcmc_run_block made) and b9_logpost_device are each the FIRST evaluating call after such a reload."""
    return [("set_options", GIVEN, 1, 2, 2), ("set_tuning", {"two_launch_steps": 1})] + conf("L", "c300") + [("block", 2, 20, True, True)] + \
        conf("P8", "c20k") + [("block", 2, 20, True, True, "off"), ("set_tuning", {})] + conf("L", "c300") + [("logpost", 2, False)] + \
        conf("P8", "c20k") + [("logpost_device", 8), ("logpost", 2, True)]


HOST_OPS = ("logpost", "sample_mass", "derive_isochrone", "sample_wd_mass")


def host_subset(steps):
    """what the CPU stand-in over the oracle can play: the configuration (tuning has no meaning there) and the four operations the
    oracle states; logpost_device counts as logpost with the per-star values"""
    out = []
    for st in steps:
        if st[0] == "logpost_device":
            st = ("logpost", st[1], True)
        if st[0] in CONFIG_OPS[:4] or st[0] in HOST_OPS:
            out.append(st)
    return out
