"""The eight reductions over a saved chain on the ragged scripts of tests/ragged_chain.py: every call against its family's
reference through its family's comparator, with the pruning and without it; every row's increment as bits, whatever the row
before it was and on whichever side of the 32-row seam it sits; a long-lived context against fresh ones after tables of every
length; and the bitwise ties between the calls on a ragged script.  What the scripts reach, that the comparison is not vacuous
and well conditioned, and which faults the comparators reject: tests/test_ragged_chain_host.py, on the CPU.

Catalogue: 140 stars, 25 of them WD-stage; scripts of 35 to 38 rows.  The tolerances are the families' own (tests/*_check.py)."""
import numpy as np
import pytest

import ragged_chain as rcn
import wdbins_ref as br
import wdmoments_check as wc
import wdmoments_ref as wr
from base_amd import abi

pytestmark = pytest.mark.gpu

COMBO_IDS = [f"{s}-k{K}q{Q}" for s, K, Q in rcn.COMBOS]
BITWISE, BITWISE_IDS = rcn.COMBOS, COMBO_IDS
CALLS = rcn.MS_CALLS + rcn.WD_CALLS + ("sample_wd_mass",)
SEED, ROW0 = 11, 100


def make_engine(combo):
    from base_amd import engine
    return engine.Engine(*rcn.device_args(rcn.problem(combo[0]), combo[1], combo[2]))


class Shared:
    """one engine at a time, kept while consecutive tests ask for the same combination"""
    combo, eng = None, None

    @classmethod
    def engine(cls, combo):
        if cls.combo != combo:
            cls.close()
            cls.combo, cls.eng = combo, make_engine(combo)
        return cls.eng

    @classmethod
    def close(cls):
        if cls.eng is not None:
            cls.eng.close()
        cls.combo, cls.eng = None, None


@pytest.fixture(scope="module", autouse=True)
def _close_the_shared_engine():
    yield
    Shared.close()
    _ALONE.clear()


def n_wd_nodes(k):
    return rcn.WD_NODES[k % 2]


# ---- the calls in one form: call(eng, name, ref, rows, n_nodes, start) -> tuple of arrays; start: None, or the tuple to continue ----
def call(eng, name, ref, rows, n_nodes, start=None, row0=ROW0):
    """The call `name` over `rows`: a tuple (accumulators ..., per-row outputs ...).  start: the accumulators of the rows before
    (continued), None: from nothing."""
    rows = np.asarray(rows).reshape(-1, abi.B9_NPARAM)
    if name == "star_moments":
        return (eng.star_moments(rows, None if start is None else start[0]),)
    if name == "pointwise":
        acc, tail, lpd = eng.pointwise(rows, rcn.TAIL, *((None, None) if start is None else start[:2]))
        return acc, tail, lpd
    if name == "mass_hist":
        return eng.mass_hist(rows, ref.hist_edges(), abi.HQ_PRIMARY, None if start is None else start[0])
    if name == "star_bins":
        return (eng.star_bins(rows, ref.bins_edges(), abi.HQ_PRIMARY, None if start is None else start[0]),)
    if name == "phot_resid":
        return eng.phot_resid(rows, None if start is None else start[0])
    if name == "wd_moments":
        return (eng.wd_moments(rows, n_nodes, None if start is None else start[0])[0],)
    if name == "wd_bins":
        edges = ref.wd_edges(n_nodes if n_nodes in rcn.WD_NODES else rcn.WD_NODES[0])[0]      # (another grid: the bitwise tests; any edges do)
        return (eng.wd_bins(rows, n_nodes, edges, abi.WQ_ALL, None if start is None else start[0])[0],)
    if name == "sample_wd_mass":
        g = eng.sample_wd_mass(rows, n_nodes, seed=SEED, row0=row0)
        return tuple(g[k] for k in ("zams", "wd_mass", "prec_log_age", "log_cool_age", "log_teff", "logg", "member", "pop"))
    raise ValueError(name)


N_ACC = {"star_moments": 1, "pointwise": 2, "mass_hist": 1, "star_bins": 1, "phot_resid": 1, "wd_moments": 1, "wd_bins": 1, "sample_wd_mass": 0}
ADDITIVE = ("star_moments", "mass_hist", "star_bins", "phot_resid", "wd_moments", "wd_bins")


def zeros_like_start(name, out):
    """what a continued call starts from when nothing came before: zeros (b9_pointwise: zeros and a tail of -inf)"""
    if name == "pointwise":
        return np.zeros_like(out[0]), np.full_like(out[1], -np.inf)
    return tuple(np.zeros_like(a) for a in out[:N_ACC[name]])


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


# ---- 1. against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(rcn.N_SCRIPTS))
@pytest.mark.parametrize("combo", rcn.COMBOS, ids=COMBO_IDS)
def test_against_the_reference(combo, k):
    """The whole script in one call, with the pruning and with marg_no_pruning = 1; b9_mass_hist, b9_phot_resid and b9_pointwise
    with their per-row outputs; b9_star_bins and b9_wd_bins on per-star edges that straddle the stars' masses; the b9_wd_* calls
    at 63 and 65 nodes (by script)."""
    ref = rcn.reference(*combo)
    prob = ref.prob
    rows, n_nodes = prob["scripts"][k], n_wd_nodes(k)
    want = rcn.ms_outputs(ref, rows)
    want.update(rcn.wd_outputs(ref, n_nodes, rows))
    eng = Shared.engine(combo)
    for pruning in (True, False):
        eng.set_tuning(**({} if pruning else {"marg_no_pruning": 1}))
        try:
            for name in rcn.MS_CALLS + rcn.WD_CALLS:
                got = call(eng, name, ref, rows, n_nodes)
                rcn.check_call(name, got[0] if len(got) == 1 else got, want[name][1], ref, pruning=pruning)
            g = eng.sample_wd_mass(rows, n_nodes, seed=SEED, row0=ROW0)
            rcn.check_wd_sample(g, want["wd_moments"][1], prob, rows, n_nodes)
        finally:
            eng.set_tuning()
    acc = call(eng, "star_moments", ref, rows, n_nodes)[0]
    n_valid = sum(rcn.row_facts(prob["pack_d"], r, combo[1], prob["n_pops"])[0] == "valid" for r in rows)
    assert np.all(acc[:, abi.MOM_ROWS] == n_valid) and n_valid <= len(rows) - 4


# ---- 2. bitwise placement ---------------------------------------------------------------------------------------------------------
_ALONE = {}


def alone(combo, ref, row, n_nodes):
    """{call: its outputs} of `row` in one-row calls, each on a context of its own that has done nothing else; kept per distinct row."""
    key = (combo, n_nodes, row.tobytes())
    if key not in _ALONE:
        _ALONE[key] = {name: on_a_fresh_context(combo, name, ref, row, n_nodes, row0=0) for name in CALLS[:-1]}
    return _ALONE[key]


def on_a_fresh_context(combo, name, ref, rows, n_nodes, **kw):
    eng = make_engine(combo)
    try:
        return call(eng, name, ref, rows, n_nodes, **kw)
    finally:
        eng.close()


@pytest.mark.parametrize("k", range(rcn.N_SCRIPTS))
@pytest.mark.parametrize("combo", BITWISE, ids=BITWISE_IDS)
def test_every_rows_increment_is_the_same_bits_wherever_it_sits(combo, k):
    """For every row j of the script: the accumulators after rows[:j + 1], started from zeros, are those after rows[:j] plus the
    row's own one-row result, one add each (b9_pointwise, whose state is no sum: the state after rows[:j + 1] is the one-row call
    continued from the state after rows[:j], and the row's row_lpd is its one-row row_lpd); the per-row outputs of the whole
    script are the rows' own; the whole script is 1 + 32 + the rest, continued; b9_sample_wd_mass draws for row j at row0 + j
    what it draws for it alone."""
    ref = rcn.reference(*combo)
    prob = ref.prob
    rows, n_nodes = prob["scripts"][k], n_wd_nodes(k)
    eng = Shared.engine(combo)
    for name in CALLS[:-1]:
        whole = call(eng, name, ref, rows, n_nodes)
        na = N_ACC[name]
        before = zeros_like_start(name, whole)
        for j in range(len(rows)):
            one = alone(combo, ref, rows[j], n_nodes)[name]
            after = call(eng, name, ref, rows[:j + 1], n_nodes, zeros_like_start(name, whole))
            if name in ADDITIVE:
                assert same(after[:na], tuple(b + o for b, o in zip(before, one[:na]))), (name, j)
            else:
                assert same(after[:na], call(eng, name, ref, rows[j], n_nodes, before)[:na]), (name, j)
            for a, w, o in zip(after[na:], whole[na:], one[na:]):                  # the per-row outputs
                assert np.array_equal(a[j], o[0]) and np.array_equal(w[j], o[0]), (name, j)
            before = after[:na]
        assert same(before, whole[:na]), name                                      # (a call from zeros continued = a call from nothing)
        part = call(eng, name, ref, rows[:1], n_nodes)
        part = call(eng, name, ref, rows[1:33], n_nodes, part[:na])
        part = call(eng, name, ref, rows[33:], n_nodes, part[:na])
        assert same(part[:na], whole[:na]), name
    batch = call(eng, "sample_wd_mass", ref, rows, n_nodes)
    assert (batch[0] > 0).any()
    for j in range(len(rows)):
        one = on_a_fresh_context(combo, "sample_wd_mass", ref, rows[j], n_nodes, row0=ROW0 + j)
        assert all(np.array_equal(b[j], o[0]) for b, o in zip(batch, one)), j


# ---- 2b. the WD family's own chunk boundary ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 4, 6])
@pytest.mark.parametrize("combo", [("base4", 1, 2), ("wdragged5", 2, 2), ("base9", 3, 2)], ids=["base4", "wdragged5", "base9"])
def test_the_wd_family_crosses_its_own_chunk_boundary(combo, k):
    """b9_sample_wd_mass, b9_wd_moments and b9_wd_bins cut their rows by a rule of their own (256 rows, 64 MiB of node tables): at
    63 or 65 nodes a script is one chunk.  At ragged_chain.wd_seam_nodes -- thousands of nodes -- the rule gives chunks of 32 rows
    and rows 31 | 32 of the script (158 -> 2 points, 2 -> 158, no isochrone -> 158, 158 -> no isochrone) straddle a chunk boundary
    inside ONE call.  No reference at that grid: the bits.  The call over the whole script is the same rows cut elsewhere by the
    caller (20 + rest, each one chunk; 1 + 32 + rest), the rows around the boundary add what they give alone on a fresh context,
    and the draws of every row are the row's own."""
    ref = rcn.reference(*combo)
    prob = ref.prob
    rows = prob["scripts"][k]
    s = prob["setting"]
    eng = Shared.engine(combo)
    for name in rcn.WD_FAMILY[1:]:
        n_nodes = rcn.wd_seam_nodes(name, s.n_filt, s.n_pops, len(prob["wd"]), rcn.WD_BINS)
        assert rcn.wd_family_chunk(name, len(rows), s.n_filt, s.n_pops, n_nodes, len(prob["wd"]), rcn.WD_BINS) == rcn.CHUNK < len(rows)
        whole = call(eng, name, ref, rows, n_nodes)
        assert (whole[0] != 0).any()
        for cut in ((20,), (1, 33)):
            part, lo = None, 0
            for hi in cut + (len(rows),):
                part = call(eng, name, ref, rows[lo:hi], n_nodes, part)
                lo = hi
            assert same(part, whole), (name, cut)
        for j in (30, 31, 32, 33):
            zero = zeros_like_start(name, whole)
            before, after = call(eng, name, ref, rows[:j], n_nodes, zero), call(eng, name, ref, rows[:j + 1], n_nodes, zero)
            one = on_a_fresh_context(combo, name, ref, rows[j], n_nodes)
            assert same(after, (before[0] + one[0],)), (name, j)
    n_nodes = rcn.wd_seam_nodes("sample_wd_mass", s.n_filt, s.n_pops)
    assert rcn.wd_family_chunk("sample_wd_mass", len(rows), s.n_filt, s.n_pops, n_nodes) == rcn.CHUNK
    batch = call(eng, "sample_wd_mass", ref, rows, n_nodes)
    assert (batch[0] > 0).any()
    for j in (0, 30, 31, 32, 33, len(rows) - 1):
        one = on_a_fresh_context(combo, "sample_wd_mass", ref, rows[j], n_nodes, row0=ROW0 + j)
        assert all(np.array_equal(b[j], o[0]) for b, o in zip(batch, one)), j


# ---- 3. the arena across calls ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", BITWISE, ids=BITWISE_IDS)
def test_a_long_lived_context_equals_fresh_ones(combo):
    """On one context: the row of the longest table, then the one-interval row, the row without isochrone and the 32-point row,
    each in a one-row call.  Every result is the same one-row call's on a context that has done nothing else, as bits -- first call
    by call, then with the eight calls interleaved row by row (they share the context's arena)."""
    import ragged_walk as rw
    ref = rcn.reference(*combo)
    prob = ref.prob
    rows = [rw._cell_row(prob["pack_d"], a, 1, 0.35) for a in (3, 9, rcn.INVALID_CELL, 7)]
    assert [rcn.row_facts(prob["pack_d"], r, combo[1], prob["n_pops"])[1] for r in rows] == [158, 2, 0, 32]
    n_nodes = rcn.WD_NODES[0]
    fresh = {}
    for name in CALLS:
        for i, r in enumerate(rows):
            eng = make_engine(combo)
            try:
                fresh[(name, i)] = call(eng, name, ref, r, n_nodes)
            finally:
                eng.close()
        assert not same(fresh[(name, 0)], fresh[(name, 1)]) and all(np.all(a == 0) or np.all(np.isneginf(a[a != 0])) for a in fresh[(name, 2)]), name
    for name in CALLS:                                                             # call by call
        eng = make_engine(combo)
        try:
            for i, r in enumerate(rows):
                assert same(call(eng, name, ref, r, n_nodes), fresh[(name, i)]), (name, i)
        finally:
            eng.close()
    eng = make_engine(combo)                                                       # interleaved
    try:
        for order in (CALLS, CALLS[::-1]):
            for i, r in enumerate(rows):
                for name in order:
                    assert same(call(eng, name, ref, r, n_nodes), fresh[(name, i)]), (name, i)
    finally:
        eng.close()


# ---- 4. the ties between the calls, on a ragged script ----------------------------------------------------------------------------
@pytest.mark.parametrize("combo", [("wdragged5", 2, 2), ("base4", 1, 2)], ids=["wdragged5-k2q2", "base4-k1q2"])
def test_the_ties_between_the_calls_hold_on_a_ragged_script(combo):
    """tests/test_gpu_chain_ties.py's membership column -- the same bits in b9_star_moments, b9_phot_resid and b9_mass_hist -- and
    tests/test_gpu_starbins.py's shared edges -- b9_star_bins on one set of edges for every star is b9_mass_hist's star_hist --
    on script 0 (158 -> 2 points across the seam); b9_wd_moments' counts and membership against b9_star_moments' at 8 K nodes at
    test_gpu_wdmoments.test_ties_to_star_moments' tolerance."""
    ref = rcn.reference(*combo)
    prob = ref.prob
    rows = prob["scripts"][0]
    eng = Shared.engine(combo)
    mom = eng.star_moments(rows)
    member = mom[:, abi.MOM_MEMBER]
    assert (member > 1.0).sum() >= 60
    star, rws = eng.phot_resid(rows)
    assert np.array_equal(star[:, 0], mom[:, abi.MOM_ROWS]) and np.array_equal(star[:, 1], member)
    wd_stage = np.asarray(prob["cl"]["stage"]) == abi.STAGE_WD
    for quantity in (abi.HQ_PRIMARY, abi.HQ_SECONDARY, abi.HQ_SYSTEM):             # the membership column, MS/RGB- and WD-stage stars
        full, _ = eng.mass_hist(rows, ref.hist_edges(), quantity, want_rows=False)
        assert np.array_equal(full[~wd_stage, -1], member[~wd_stage]) and np.array_equal(full[wd_stage, -1], member[wd_stage]), quantity
    edges = np.ascontiguousarray(ref.hist_edges()[2:-2])                           # 29 bins (b9_star_bins takes up to 30); weight outside them
    hist, _ = eng.mass_hist(rows, edges, abi.HQ_PRIMARY, want_rows=False)
    nb = len(edges) - 1
    assert np.array_equal(hist[:, nb], member)
    acc = eng.star_bins(rows, np.tile(edges, (prob["n_stars"], 1)), abi.HQ_PRIMARY)
    assert np.array_equal(acc[:, 1:nb + 1], hist[:, :nb]) and np.array_equal(acc[:, nb + 2], member)
    assert (acc[:, 0] > 0).any() and (acc[:, nb + 1] > 0).any()
    pw, _, _ = eng.pointwise(rows)
    assert np.array_equal(pw[:, abi.PW_ROWS], mom[:, abi.MOM_ROWS])                # (every star has a node in every valid row)
    n8 = 8 * combo[1]
    wdm, idx = eng.wd_moments(rows, n8)
    mine = wdm[:, [wr.ROWS, wr.MEMBER, wr.M1, wr.M1SQ, wr.POP1]]
    theirs = mom[idx][:, [abi.MOM_ROWS, abi.MOM_MEMBER, abi.MOM_M1, abi.MOM_M1SQ, abi.MOM_POP1]]
    np.testing.assert_allclose(mine, theirs, rtol=wc.TIE_RTOL, atol=0)
    wdb, _ = eng.wd_bins(rows, n8, ref.wd_edges(rcn.WD_NODES[0])[0])
    for s in range(br.N_Q):                                                        # the total of every line, bit for bit
        assert np.array_equal(wdb[:, s, -1], wdm[:, wr.MEMBER]), br.NAMES[s]
