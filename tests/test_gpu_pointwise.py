"""b9_pointwise (the modelScore counterpart) on the GPU: the per-star state, the tail and the row sums against the numpy
statement tests/pointwise_ref.py; v itself against b9_logpost's per-star values; the edges of the star, node and filter shapes;
special stars; the reducers in isolation on the device's own v matrix; bit-for-bit invariances; the sampler left alone; the
errors; the power to tell two populations from one; the CLI.  Each test makes its own short-lived engine on the small packs of
build_problem(small=True); a case's reference is computed once and shared.

Tolerances: tests/pointwise_check.py."""
import ctypes as C
import functools
import math
import os
import shutil

import numpy as np
import pytest

import pointwise_check as pc
import pointwise_ref as pr
import test_gpu_moments as tm
from base_amd import abi, synth
from conftest import build_problem
from cli_util import cli as _cli

pytestmark = pytest.mark.gpu
_dp = C.POINTER(C.c_double)
T_REF = 2                                                 # the tail kept in the comparisons with the reference (3 rows)


def make_engine(pack, stars, priors, n_pops, K, Q, mode=abi.MODE_GIVEN_MASS):
    from base_amd import engine
    return engine.Engine(pack, stars, priors, tm.opts(n_pops, K, Q, mode))


def reference(pack_d, cl, rows, n_pops, K, Q):
    V, inside, live = pr.v_matrix(pack_d, cl, rows, n_pops, K, Q)
    return V, inside, live, pr.accumulate(V, inside), pr.top_tail(V, inside, T_REF), pr.row_sums(V, inside)


def against_reference(pack_d, cl, pack, stars, priors, n_pops, K, Q, rows, ref=None):
    """All three outputs, with the pruning and without it, against the reference; returns (acc, tail, row_lpd, reference)."""
    ref = ref or reference(pack_d, cl, rows, n_pops, K, Q)
    V, inside, live, want_acc, want_tail, want_rows = ref
    eng = make_engine(pack, stars, priors, n_pops, K, Q)
    try:
        got = eng.pointwise(rows, T_REF)
        eng.set_tuning(marg_no_pruning=1)
        full = eng.pointwise(rows, T_REF)
        eng.set_tuning()
    finally:
        eng.close()
    n = V.shape[1]
    for what, (acc, tail, rws) in (("pruned", got), ("unpruned", full)):
        print(f"{what}: largest difference VMAX {pc.largest(acc[:, pr.VMAX], want_acc[:, pr.VMAX]):.3g}, MEAN "
              f"{pc.largest(acc[:, pr.MEAN], want_acc[:, pr.MEAN]):.3g}, M2 {pc.largest(acc[:, pr.M2], want_acc[:, pr.M2]):.3g}, "
              f"tail {pc.largest(tail, want_tail):.3g}, row_lpd / n {pc.largest(rws / n, want_rows / n):.3g}")
        pc.assert_acc(acc, want_acc)
        pc.assert_tail(tail, want_tail)
        pc.assert_rows(rws, want_rows, n)
    return got + (ref,)


@functools.lru_cache(maxsize=None)
def case(k):
    """Case k of test_gpu_moments.CASES with its rows (3 + one outside the grid) and the reference, built once."""
    name, n_filt, n_y, n_pops, K, Q, n_stars, wd_frac, n_nodes = tm.CASES[k]
    pack_d, cl, pack, stars, priors, _ = build_problem(name, n_filt, n_stars=n_stars, wd_frac=wd_frac, n_y=n_y, n_pops=n_pops, seed=12)
    rows = tm.rows_for(pack_d, cl, n_pops)
    rows.setflags(write=False)
    return pack_d, cl, pack, stars, priors, rows, reference(pack_d, cl, rows, n_pops, K, Q)


@functools.lru_cache(maxsize=None)
def small():
    """parsec, 4 filters, 70 stars (WD-stage among them), one population, 2 x 2 grid, 3 rows + one outside."""
    pack_d, cl, pack, stars, priors, _ = build_problem("parsec", 4, n_stars=70, wd_frac=0.1, seed=12)
    rows = tm.rows_for(pack_d, cl, 1)
    rows.setflags(write=False)
    return pack_d, cl, pack, stars, priors, rows


# ---- 1. parity with the reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(4), ids=[f"{c[0]}{c[1]}" for c in tm.CASES])
def test_parity_with_reference(k):
    name, n_filt, n_y, n_pops, K, Q, n_stars, wd_frac, n_nodes = tm.CASES[k]
    pack_d, cl, pack, stars, priors, rows, ref = case(k)
    V, inside, live, want_acc, want_tail, want_rows = ref
    # not vacuous: stated on the reference before the device is consulted
    m2, wd = pc.non_vacuity(want_acc, cl, live)
    print(f"{name} {n_filt}: {m2} of {n_stars} stars with M2 > 0, {wd} live WD-stage stars")
    assert m2 >= (9 * n_stars + 9) // 10 and list(inside) == [True, True, True, False]
    if wd_frac > 0:
        assert wd >= 1
    acc, tail, rws, _ = against_reference(pack_d, cl, pack, stars, priors, n_pops, K, Q, rows, ref)
    assert acc.shape == (n_stars, 8) and tail.shape == (n_stars, T_REF) and rws.shape == (4,)
    assert np.all(acc[:, pr.ROWS] == 3) and np.all(acc[:, pr.NINF] == 0)     # the row outside the grid adds nothing to any star
    assert rws[3] == -np.inf and np.all(np.isfinite(rws[:3]))


# ---- 2. v itself ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1])
def test_v_is_the_marginalised_per_star_value(k):
    """A one-row call's VMAX column is v: against the reference, and against b9_logpost's out_perstar in marginalised mode on
    the same grid (another kernel, another summation order: the project tolerance); row_lpd against the sum of that out_perstar."""
    name, n_filt, n_y, n_pops, K, Q, n_stars, wd_frac, n_nodes = tm.CASES[k]
    pack_d, cl, pack, stars, priors, rows, ref = case(k)
    V = ref[0]
    eng = make_engine(pack, stars, priors, n_pops, K, Q, abi.MODE_MARGINALISED)
    try:
        for r in range(2):
            acc, _, rws = eng.pointwise(rows[r:r + 1])
            _, ps = eng.logpost(rows[r:r + 1], perstar=True)
            assert np.all(acc[:, pr.ROWS] == 1) and np.all(acc[:, pr.SPOS] == 1) and np.array_equal(acc[:, pr.RMAX], -acc[:, pr.VMAX])
            assert np.array_equal(acc[:, pr.MEAN], acc[:, pr.VMAX]) and np.all(acc[:, pr.M2] == 0)
            print(f"row {r}: largest difference to the reference {pc.largest(acc[:, pr.VMAX], V[r]):.3g}, to b9_logpost {pc.largest(acc[:, pr.VMAX], ps[0]):.3g}")
            pc.assert_values(acc[:, pr.VMAX], V[r])
            pc.assert_values(acc[:, pr.VMAX], ps[0])
            pc.assert_rows(rws, np.array([ps[0].sum()]), n_stars)
    finally:
        eng.close()


# ---- 3. edges of the shapes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_wd", [0, 1, 4, 5])
@pytest.mark.parametrize("n_ms", [1, 64, 65])
def test_star_count_edges(n_ms, n_wd):
    pack_d, cl, pack, _, priors, _ = build_problem("parsec", 4, n_stars=400, wd_frac=0.1, seed=12)
    stage = np.asarray(cl["stage"])
    ms, wd = np.flatnonzero(stage != abi.STAGE_WD)[:n_ms], np.flatnonzero(stage == abi.STAGE_WD)[:n_wd]
    assert len(ms) == n_ms and len(wd) == n_wd
    cl = tm.subset(cl, np.sort(np.concatenate([ms, wd])))
    acc, _, _, _ = against_reference(pack_d, cl, pack, abi.make_stars(cl), priors, 1, 2, 2, tm.rows_for(pack_d, cl, 1, 2))
    assert np.all(acc[:, pr.ROWS] == 2)


@pytest.mark.parametrize("n_pops", [1, 2])
@pytest.mark.parametrize("n_filt", [4, 5, 8, 9, 16])
def test_every_instance(n_filt, n_pops):
    """The six instances, and 5 and 9 filters: padded rows on both sides of the 8 | 16 seam."""
    pack_d, cl, pack, stars, priors, _ = build_problem("dsed", n_filt, n_stars=70, wd_frac=0.1, n_y=3 if n_pops == 2 else 1, n_pops=n_pops, seed=12)
    rows = tm.rows_for(pack_d, cl, n_pops, 2, outside=False)
    acc, _, rws, ref = against_reference(pack_d, cl, pack, stars, priors, n_pops, 2, 2, rows)
    assert np.all(acc[:, pr.ROWS] == 2) and np.all(np.isfinite(rws)) and ref[2].all(axis=0).sum() >= 60


@pytest.mark.parametrize("n_eep,K,n_chunks", [(40, 1, 1), (90, 3, 5)])
def test_node_table_edges(n_eep, K, n_chunks):
    """One partial 64-node chunk; five chunks, the last one partial."""
    pack_d, cl, pack, stars, priors, _ = build_problem("parsec", 4, n_stars=70, wd_frac=0.1, seed=12, n_eep=n_eep)
    assert ((int(np.max(pack_d["iso_n_eep"])) - 1) * K + 63) // 64 == n_chunks
    against_reference(pack_d, cl, pack, stars, priors, 1, K, 2, tm.rows_for(pack_d, cl, 1))


# ---- 4. special stars -------------------------------------------------------------------------------------------------------
def field_term_as_staged(cl, i):
    """log(1 - p) + log fs with the sums in the order the catalogue is staged in: log fs = ((0 - log r_0) - log r_1) - ..."""
    log_fs = 0.0
    for lo, hi in zip(np.asarray(cl["filter_prior_min"]), np.asarray(cl["filter_prior_max"])):
        log_fs -= math.log(float(hi) - float(lo))
    return math.log1p(-float(cl["clust_prior"][i])) + log_fs


def test_special_stars():
    """A star with every filter unused (its v is the prior's integral over the grid mixed with the field term) and one with (all
    but) no membership prior (b9_load_stars refuses 0): v = la to rounding."""
    pack_d, cl, pack, _, priors, _ = build_problem("parsec", 4, n_stars=70, wd_frac=0.1, seed=12)
    cl = tm.subset(cl, np.arange(70))
    cl["sigma"] = np.array(cl["sigma"], dtype=np.float64)
    cl["clust_prior"] = np.array(cl["clust_prior"], dtype=np.float64)
    ms = np.flatnonzero((np.asarray(cl["stage"]) != abi.STAGE_WD) & (cl["sigma"] > 0).all(axis=1))
    cl["sigma"][ms[3]] = -1.0
    cl["clust_prior"][ms[5]] = 1e-300
    rows = tm.rows_for(pack_d, cl, 1)
    acc, tail, rws, ref = against_reference(pack_d, cl, pack, abi.make_stars(cl), priors, 1, 2, 2, rows)
    la = field_term_as_staged(cl, ms[5])
    assert acc[ms[5], pr.ROWS] == 3 and abs(acc[ms[5], pr.VMAX] - la) <= 1e-12 * abs(la) and acc[ms[5], pr.M2] <= 1e-20
    assert acc[ms[3], pr.ROWS] == 3 and np.isfinite(acc[ms[3], pr.VMAX]) and acc[ms[3], pr.VMAX] > field_term_as_staged(cl, ms[3])


def test_wd_stage_star_without_a_live_node():
    """A parametrised IFMR that gives M_wd <= 0 at every node (stated on the reference first): a WD-stage star at prior 0.5 has
    v = the field term exactly and the row counts; at prior 1 the row is a -inf row -- NINF = 1, the finite columns untouched,
    row_lpd = -inf."""
    pack_d, cl, pack, _, priors, _ = build_problem("parsec", 4, n_stars=70, wd_frac=0.1, seed=12, ifmr_id=abi.IFMR_LINEAR)
    cl = tm.subset(cl, np.arange(70))
    cl["clust_prior"] = np.array(cl["clust_prior"], dtype=np.float64)
    wd = np.flatnonzero(np.asarray(cl["stage"]) == abi.STAGE_WD)
    half, one = wd[0], wd[1]
    cl["clust_prior"][half] = 0.5
    rows = np.array(tm.rows_for(pack_d, cl, 1, 3, outside=False))
    rows[1, abi.P_IFMR_INTERCEPT], rows[1, abi.P_IFMR_SLOPE] = -10.0, 0.0
    V, inside, live = pr.v_matrix(pack_d, cl, rows, 1, 2, 2)
    assert inside.all() and not live[1, wd].any() and live[0, wd].all() and live[2, wd].all()
    stars = abi.make_stars(cl)
    acc, tail, rws, _ = against_reference(pack_d, cl, pack, stars, priors, 1, 2, 2, rows, (V, inside, live, pr.accumulate(V, inside),
                                                                                           pr.top_tail(V, inside, T_REF), pr.row_sums(V, inside)))
    assert np.all(acc[:, pr.ROWS] == 3) and np.all(acc[:, pr.NINF] == 0) and np.all(np.isfinite(rws))
    eng = make_engine(pack, stars, priors, 1, 2, 2)
    try:
        a1, _, r1 = eng.pointwise(rows[1:2])
    finally:
        eng.close()
    assert a1[half, pr.ROWS] == 1 and a1[half, pr.VMAX] == field_term_as_staged(cl, half) == V[1, half]
    # ... and at membership prior 1
    cl["clust_prior"][one] = 1.0
    stars = abi.make_stars(cl)
    eng = make_engine(pack, stars, priors, 1, 2, 2)
    try:
        a0, t0, r0 = eng.pointwise(rows[0:1], 2)
        a01, t01, r01 = eng.pointwise(rows[1:2], 2, a0, t0)
        whole, tw, rw = eng.pointwise(rows, 2)
    finally:
        eng.close()
    assert a0[one, pr.ROWS] == 1 and a0[one, pr.NINF] == 0 and np.isfinite(a0[one, pr.VMAX])
    assert a01[one, pr.ROWS] == 2 and a01[one, pr.NINF] == 1 and np.array_equal(a01[one, pr.VMAX:], a0[one, pr.VMAX:])
    assert np.array_equal(t01[one], t0[one]) and r01[0] == -np.inf and np.isfinite(r0[0])
    assert whole[one, pr.ROWS] == 3 and whole[one, pr.NINF] == 1 and rw[1] == -np.inf and np.isfinite(rw[0]) and np.isfinite(rw[2])
    assert np.isfinite(tw[one, 1]) and np.all(whole[np.arange(70) != one, pr.NINF] == 0)
    V1, inside1, _ = pr.v_matrix(pack_d, cl, rows, 1, 2, 2)
    assert V1[1, one] == -np.inf
    pc.assert_acc(whole, pr.accumulate(V1, inside1))
    pc.assert_tail(tw, pr.top_tail(V1, inside1, 2))
    pc.assert_rows(rw, pr.row_sums(V1, inside1), 70)


# ---- 5. the reducers in isolation ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_matrix():
    """Case 1, 40 rows (some repeated: ties), and the device's own v matrix from 40 single-row calls."""
    pack_d, cl, pack, stars, priors, _, _ = case(0)
    rows = synth.walker_params(cl["truth"], 40, seed=8, scale=0.3, n_pops=2)
    rows[:, abi.P_LAMBDA] = np.clip(rows[:, abi.P_LAMBDA], 0.05, 0.95)
    rows[[5, 17, 18, 33]] = rows[[2, 2, 11, 30]]
    eng = make_engine(pack, stars, priors, 2, 2, 2)
    try:
        V, lpd = np.empty((40, eng.n_stars)), np.empty(40)
        for r in range(40):
            acc, _, rws = eng.pointwise(rows[r:r + 1])
            assert np.all(acc[:, pr.ROWS] == 1) and np.all(acc[:, pr.NINF] == 0)
            V[r], lpd[r] = acc[:, pr.VMAX], rws[0]
    finally:
        eng.close()
    rows.setflags(write=False); V.setflags(write=False)
    return rows, V, lpd


def test_accumulate_and_rows_on_the_device_matrix():
    pack_d, cl, pack, stars, priors, _, _ = case(0)
    rows, V, lpd = device_matrix()
    eng = make_engine(pack, stars, priors, 2, 2, 2)
    try:
        acc, _, rws = eng.pointwise(rows)
    finally:
        eng.close()
    want = pr.accumulate(V)
    assert np.array_equal(acc[:, :2], want[:, :2]) and np.all(acc[:, 0] == 40)
    assert np.array_equal(acc[:, pr.VMAX], V.max(axis=0)) and np.array_equal(acc[:, pr.RMAX], (-V).max(axis=0))
    np.testing.assert_allclose(acc, want, rtol=1e-12, atol=0)
    assert np.array_equal(rws, lpd) and np.array_equal(rws, pr.row_sums(V, np.ones(40, bool)))      # the sequential sum, bit for bit


@pytest.mark.parametrize("T", [1, 2, 31, 32, 33, 256])
def test_tail_on_the_device_matrix(T):
    pack_d, cl, pack, stars, priors, _, _ = case(0)
    rows, V, _ = device_matrix()
    eng = make_engine(pack, stars, priors, 2, 2, 2)
    try:
        _, tail, _ = eng.pointwise(rows, T, want_rows=False)
        _, rev, _ = eng.pointwise(rows[::-1], T, want_rows=False)
    finally:
        eng.close()
    want = np.full((V.shape[1], T), -np.inf)
    srt = np.sort(-V, axis=0)[::-1][:T].T
    want[:, :srt.shape[1]] = srt
    assert (np.diff(np.sort(-V, axis=0), axis=0) == 0).sum() >= 4 * V.shape[1]          # the repeated rows are ties
    assert np.array_equal(tail, want) and np.array_equal(rev, want)


# ---- 6. bitwise invariances -------------------------------------------------------------------------------------------------
def test_bitwise_invariances():
    pack_d, cl, pack, stars, priors, _, _ = case(0)
    rows = np.array(device_matrix()[0][:33])
    T = 5
    eng = make_engine(pack, stars, priors, 2, 2, 2)
    try:
        whole = eng.pointwise(rows, T)
        assert np.all(whole[0][:, pr.ROWS] == 33) and (whole[0][:, pr.M2] > 0).sum() >= 120
        for cuts in ((1,), (20,), tuple(range(1, 33))):    # 1 + 32, 20 + 13, 33 single rows: one row over the 32-row chunk seam
            acc = tail = None
            lpd = []
            for a, b in zip((0,) + cuts, cuts + (33,)):
                acc, tail, r = eng.pointwise(rows[a:b], T, acc, tail)
                lpd.append(r)
            assert np.array_equal(acc, whole[0]) and np.array_equal(tail, whole[1]) and np.array_equal(np.concatenate(lpd), whole[2])
        # the rows reversed: the same multiset per star, the row sums reversed
        rev = eng.pointwise(rows[::-1], T)
        assert np.array_equal(rev[1], whole[1]) and np.array_equal(rev[2], whole[2][::-1])
        assert np.array_equal(rev[0][:, [pr.ROWS, pr.NINF, pr.VMAX, pr.RMAX]], whole[0][:, [pr.ROWS, pr.NINF, pr.VMAX, pr.RMAX]])
        # acc is the same with or without the tail and the row sums; the row sums alone
        only = eng.pointwise(rows, 0, want_rows=False)
        assert only[1] is None and only[2] is None and np.array_equal(only[0], whole[0])
        lpd = np.zeros(33)
        eng._check(eng.lib.b9_pointwise(eng._ctx, rows.ctypes.data_as(_dp), 33, 0, 0, None, None, lpd.ctypes.data_as(_dp)))
        assert np.array_equal(lpd, whole[2])
        # a row outside the grid in the middle of a batch changes nothing but its own row sum
        outside = rows[:1].copy(); outside[0, abi.P_LOGAGE] = pack_d["log_age"][-1] + 1.0
        mixed = eng.pointwise(np.concatenate([rows[:7], outside, rows[7:]]), T)
        assert np.array_equal(mixed[0], whole[0]) and np.array_equal(mixed[1], whole[1])
        assert mixed[2][7] == -np.inf and np.array_equal(np.delete(mixed[2], 7), whole[2])
        # a repeated call; the siblings in between leave nothing behind
        eng.star_moments(rows[:7]); eng.phot_resid(rows[:5])
        again = eng.pointwise(rows, T)
        assert all(np.array_equal(a, b) for a, b in zip(again, whole))
    finally:
        eng.close()
    eng = make_engine(pack, stars, priors, 2, 2, 2)                           # a fresh context
    try:
        fresh = eng.pointwise(rows, T)
        assert all(np.array_equal(a, b) for a, b in zip(fresh, whole))
    finally:
        eng.close()


def test_scratch_rule_picks_the_chunk():
    """The one case above the suite's 70 - 130 stars: the chunk is forced below 32 rows by the siblings' knob, the catalogue's
    size, and one double per (row, star) needs more than 65536 stars for that.  70000 stars: a row's values take 560 kB, so the
    16 MiB rule allows 29 rows a chunk.  33 rows in one call (29 + 4) = 16 + 17 continued (chunks of 16 and 17, under both
    limits).  One-by-two grid, 4 filters: 0.1 s."""
    pack_d, cl, pack, stars, priors, _ = build_problem("parsec", 4, n_stars=70000, wd_frac=0.02, seed=12)
    assert (16 << 20) // (8 * 70000) == 29
    rows = synth.walker_params(cl["truth"], 33, seed=8, scale=0.3)
    eng = make_engine(pack, stars, priors, 1, 1, 2)
    try:
        whole = eng.pointwise(rows, 3)
        acc, tail, r0 = eng.pointwise(rows[:16], 3)
        acc, tail, r1 = eng.pointwise(rows[16:], 3, acc, tail)
    finally:
        eng.close()
    assert np.all(whole[0][:, pr.ROWS] == 33) and (whole[0][:, pr.M2] > 0).sum() >= 60000
    assert np.array_equal(acc, whole[0]) and np.array_equal(tail, whole[1]) and np.array_equal(np.concatenate([r0, r1]), whole[2])


# ---- 7. leaves the sampler alone --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [abi.MODE_GIVEN_MASS, abi.MODE_MARGINALISED])
def test_sampler_blocks_are_untouched(mode):
    from base_amd import mcmc
    pack_d, cl, pack, stars, priors, _, _ = case(1)
    free = np.array(mcmc.DEFAULT_FREE)
    chol = np.diag([mcmc.DEFAULT_STEP[k] for k in free]) * 0.3
    start = synth.walker_params(cl["truth"], 4, seed=2, scale=0.3)
    rows = tm.rows_for(pack_d, cl, 1)

    def run(interleave):
        eng = make_engine(pack, stars, priors, 1, 1, 4, mode)
        try:
            lp0 = eng.logpost(start)
            h = eng.mcmc_submit(start, lp0, np.arange(4), free, chol, 11, 0, 6, asynchronous=True)
            if interleave:
                with pytest.raises(Exception) as e:                        # B9_ERR_STATE: a block is outstanding
                    eng.pointwise(rows, 2)
                assert e.value.code == abi.B9_ERR_STATE and "outstanding" in str(e.value)
            first = [np.array(x) for x in eng.mcmc_collect(h)[:4]]
            if interleave:
                acc, _, _ = eng.pointwise(rows, 2)
                assert np.all(acc[:, pr.ROWS] == 3)
            h = eng.mcmc_submit(start, lp0, np.arange(4), free, chol, 11, 6, 6, cont=True, asynchronous=True)
            second = [np.array(x) for x in eng.mcmc_collect(h)[:4]]
        finally:
            eng.close()
        return first + second

    for a, b in zip(run(False), run(True)):
        assert np.array_equal(a, b)


# ---- 8. errors ----------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_untouched():
    from base_amd import mcmc
    pack_d, cl, pack, stars, priors, rows = small()
    eng = make_engine(pack, stars, priors, 1, 2, 2)
    try:
        n = eng.n_stars
        rows = np.ascontiguousarray(rows)

        def call(n_rows=4, acc=True, tail=True, rws=True, params=True, ctx=True, tail_len=3):
            a, t, r = np.full((n, 8), 7.25), np.full((n, 256), 7.25), np.full(4, 7.25)
            code = eng.lib.b9_pointwise(eng._ctx if ctx else None, rows.ctypes.data_as(_dp) if params else None, n_rows, 0, tail_len,
                                        a.ctypes.data_as(_dp) if acc else None, t.ctypes.data_as(_dp) if tail else None,
                                        r.ctypes.data_as(_dp) if rws else None)
            assert code == abi.B9_OK or (np.all(a == 7.25) and np.all(t == 7.25) and np.all(r == 7.25))
            return code

        assert call() == abi.B9_OK
        assert call(n_rows=0) == abi.B9_ERR_INVALID and call(n_rows=-2) == abi.B9_ERR_INVALID
        assert call(params=False) == abi.B9_ERR_INVALID
        assert call(ctx=False) == abi.B9_ERR_INVALID
        assert call(acc=False, tail=False, rws=False) == abi.B9_ERR_INVALID
        assert call(tail_len=-1) == abi.B9_ERR_INVALID and call(tail_len=257) == abi.B9_ERR_INVALID
        assert call(acc=False) == abi.B9_ERR_INVALID                       # tail without acc
        assert call(tail_len=256) == abi.B9_OK and call(tail_len=0) == abi.B9_OK
        assert call(acc=False, tail=False) == abi.B9_OK and call(rws=False) == abi.B9_OK and call(tail=False, tail_len=0) == abi.B9_OK
        # an outstanding sampler block
        free = np.array(mcmc.DEFAULT_FREE)
        chol = np.diag([mcmc.DEFAULT_STEP[k] for k in free]) * 0.3
        start = synth.walker_params(cl["truth"], 4, seed=2, scale=0.3)
        h = eng.mcmc_submit(start, eng.logpost(start), np.arange(4), free, chol, 11, 0, 6, asynchronous=True)
        assert call() == abi.B9_ERR_STATE
        eng.mcmc_collect(h)
        assert call() == abi.B9_OK
    finally:
        eng.close()


# ---- 9. power -----------------------------------------------------------------------------------------------------------------
def test_two_populations_are_told_from_one():
    """A two-population cluster, lambda = 0.5, the two Y values at the ends of a 3-point Y axis.  Eight rows near the truth scored
    with n_pops = 2 against the same rows, Y at Y_A, scored with n_pops = 1: the reference says delta elpdLoo > 5 se, and the
    device's accumulators through the host tables give the same delta and se."""
    from base_amd import hostlib
    pack_d = synth.make_pack("dsed", n_filt=5, n_y=3, n_feh=4, n_age=8, n_eep=90)
    truth = synth.default_params(pack_d)
    truth[abi.P_Y], truth[abi.P_Y2], truth[abi.P_LAMBDA] = pack_d["y"][0], pack_d["y"][-1], 0.5
    cl = synth.make_cluster(pack_d, 100, seed=12, truth=truth, wd_frac=0.05, n_pops=2)
    rows2 = synth.walker_params(truth, 8, seed=3, scale=0.1, n_pops=2)
    rows1 = rows2.copy(); rows1[:, abi.P_Y] = pack_d["y"][0]
    T = 2                                                 # min(floor(8 / 5), ceil(3 sqrt 8)) + 1
    ref = {}
    for n_pops, rows in ((2, rows2), (1, rows1)):
        V, inside, _ = pr.v_matrix(pack_d, cl, rows, n_pops, 2, 2)
        assert inside.all()
        ref[n_pops] = pr.table(V, inside, n_keep=T)[0]
    want = pr.compare(ref[2], ref[1])
    print(f"reference: delta elpdLoo = {want[1]:.3f} +- {want[2]:.3f}, delta elpdWaic = {want[3]:.3f} +- {want[4]:.3f}")
    assert want[0] == 100 and want[1] > 5 * want[2] > 0
    pack, stars = abi.make_pack(pack_d), abi.make_stars(cl)
    tab = {}
    for n_pops, rows in ((2, rows2), (1, rows1)):
        eng = make_engine(pack, stars, synth.default_priors(pack_d, truth, n_pops), n_pops, 2, 2)
        try:
            acc, tail, _ = eng.pointwise(rows, T)
        finally:
            eng.close()
        tab[n_pops] = hostlib.pointwise_table(acc, tail)
        pc.assert_table(tab[n_pops], ref[n_pops])
    ids = [str(i) for i in range(100)]
    got = hostlib.score_compare(tab[2], ids, tab[1], ids)
    assert got["nStars"] == want[0] == 100 and got["nDropped"] == want[5] == 0
    np.testing.assert_allclose([got[k] for k in hostlib.SCORE_COMPARE[1:5]], want[1:5], rtol=1e-9)


# ---- 10. the CLI --------------------------------------------------------------------------------------------------------------
def test_cli_model_score(tmp_path):
    """simCluster (200 stars) -> scatterCluster -> singlePopMcmc (short, 4 walkers x 100 main-run rows: the program passes them in
    two batches, the second continued) -> modelScore --perRow: the three files parse and equal what Engine.pointwise in ONE call
    gives through the host tables; the totals are the column sums; the same chain scored under another IFMR is a second base,
    compared with --compareTo."""
    from base_amd import build, engine, host_build, hostlib
    build.build_hip()
    host_build.build_host()
    K = Q = 4                                            # the program's defaults
    pack_d = synth.make_pack("parsec", 8, n_feh=4, n_age=8, n_eep=90)
    truth = synth.default_params(pack_d)
    truth[abi.P_IFMR_INTERCEPT], truth[abi.P_IFMR_SLOPE], truth[abi.P_IFMR_QUAD] = 0.77, 0.08, 0.0   # the session's defaults
    root = synth.write_models_dir(pack_d, str(tmp_path / "models"))
    base = str(tmp_path / "run")
    y_true = synth.write_yaml(str(tmp_path / "truth.yaml"), base + ".sim.scatter", root, base, truth, seed=17)
    r = _cli("simCluster", "--config", y_true, "--nStars", "200", "--percentBinary", "30", "--minMass", "0.4")
    assert r.returncode == 0, r.stderr
    r = _cli("scatterCluster", "--config", y_true, "--sigmaFloor", "0.01", "--sigmaAtLimit", "0.05", "--faintLimit", "45")
    assert r.returncode == 0, r.stderr
    start = truth.copy()
    start[abi.P_LOGAGE] += 0.004; start[abi.P_MOD] += 0.01; start[abi.P_FEH] -= 0.01
    fit = str(tmp_path / "fit")
    y = synth.write_yaml(str(tmp_path / "fit.yaml"), base + ".sim.scatter", root, fit, start, burn=300, run=100, walkers=4)
    r = _cli("singlePopMcmc", "--config", y, "--priorFe_H", repr(float(truth[abi.P_FEH])), "--priorDistMod", repr(float(truth[abi.P_MOD])),
             "--priorAv", repr(float(truth[abi.P_ABS])))
    assert r.returncode == 0, r.stderr
    r = _cli("modelScore", "--config", y, "--perRow")
    assert r.returncode == 0, r.stderr
    assert "star rows/s" in r.stderr and "elpd (PSIS-LOO)" in r.stdout

    cl = tm._read_phot(base + ".sim.scatter")
    phot_ids = [ln.split()[0] for ln in open(base + ".sim.scatter").read().splitlines()[1:]]
    rows = hostlib.read_res_rows(fit + ".res", start, 3)
    S = len(rows)
    assert S == 100 * 4                                   # more than one batch of 256
    T = min(256, min(S // 5, math.ceil(3 * math.sqrt(S))) + 1)
    assert T == 61
    eng = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cl), synth.default_priors(pack_d, truth), tm.opts(1, K, Q))
    try:
        acc, tail, lpd = eng.pointwise(rows, T)
    finally:
        eng.close()
    ids, cols, tab = hostlib.read_pointwise(fit + ".pointwise")
    assert ids == phot_ids and cols == list(hostlib.POINTWISE_COLUMNS)
    assert np.array_equal(tab, hostlib.pointwise_table(acc, tail), equal_nan=True)
    assert np.all(tab[:, pr.T_ROWS] == S) and np.all(tab[:, pr.T_NINF] == 0) and np.isfinite(tab[:, pr.T_K]).sum() >= 150
    assert np.array_equal(hostlib.read_row_lpd(fit + ".rowLpd"), lpd) and np.all(np.isfinite(lpd))
    tot = hostlib.read_named_values(fit + ".modelScore")
    assert list(tot) == list(hostlib.SCORE_TOTALS) and tot == hostlib.score_totals(tab)
    # the totals are the column sums
    assert tot["nStars"] == len(ids)
    for name, col in (("lppd", pr.T_LPPD), ("elpdWaic", pr.T_ELPD_WAIC), ("elpdLoo", pr.T_ELPD_LOO), ("pWaic", pr.T_PWAIC), ("pLoo", pr.T_PLOO)):
        assert tot[name] == pytest.approx(tab[:, col].sum(), rel=1e-12), name
    assert tot["elpdLooSe"] == pytest.approx(math.sqrt(len(ids) * tab[:, pr.T_ELPD_LOO].var(ddof=1)), rel=1e-12)
    assert tot["nHighK"] == (tab[:, pr.T_K] > 0.7).sum() and tot["nInfStars"] == 0
    assert tot["elpdLoo"] <= tot["lppd"] and tot["pWaic"] > 0

    # the same chain under another IFMR: a second base, then the comparison (no GPU needed for it)
    other = str(tmp_path / "other")
    shutil.copy(fit + ".res", other + ".res")
    r = _cli("modelScore", "--config", y, "--outputFileBase", other, "--ifmr", "2")
    assert r.returncode == 0, r.stderr
    ids2, _, tab2 = hostlib.read_pointwise(other + ".pointwise")
    assert ids2 == ids and not os.path.exists(other + ".rowLpd")
    r = _cli("modelScore", "--config", y, "--compareTo", other)
    assert r.returncode == 0, r.stderr
    cmp_ = hostlib.read_named_values(fit + ".modelCompare")
    assert cmp_ == hostlib.score_compare(tab, ids, tab2, ids2)
    assert cmp_["dElpdLoo"] == pytest.approx((tab[:, pr.T_ELPD_LOO] - tab2[:, pr.T_ELPD_LOO]).sum(), rel=1e-9, abs=1e-12)
    assert "delta elpd (PSIS-LOO)" in r.stdout
