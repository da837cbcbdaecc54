"""b9_star_influence (the starInfluence counterpart) on the GPU: the per-star state, the tail and the groups' sums against the
numpy statement tests/influence_ref.py; the reducers in isolation on the device's own v matrix; the ties to b9_pointwise, bit
for bit; the edges of the star, row, quantity and group shapes; bit-for-bit invariances; a -inf row; the sampler left alone;
the errors; the power to find the star that drives the age; the CLI.  Each test makes its own short-lived engine on the small
packs of build_problem(small=True); a case's reference values are test_gpu_pointwise's, computed once and shared.

Tolerances: tests/influence_check.py."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import influence_check as ic
import influence_ref as ir
import pointwise_ref as pr
import test_gpu_moments as tm
import test_gpu_pointwise as tp
from base_amd import abi, synth
from conftest import build_problem
from cli_util import cli as _cli

pytestmark = pytest.mark.gpu
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
T_REF = 2
make_engine = tp.make_engine


def quantities(n_rows, Q, seed=5):
    """The caller's per-row scalars: the library gives them no meaning, so the tests draw them."""
    return np.random.default_rng(seed).standard_normal((n_rows, Q))


def stage_groups(cl):
    """ms = 0, wd = 1: the program's default groups."""
    return (np.asarray(cl["stage"]) == abi.STAGE_WD).astype(np.int32)


def same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


# ---- 1. parity with the reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(4), ids=[f"{c[0]}{c[1]}" for c in tm.CASES])
def test_parity_with_reference(k):
    name, n_filt, n_y, n_pops, K, Q, n_stars, wd_frac, n_nodes = tm.CASES[k]
    pack_d, cl, pack, stars, priors, rows, ref = tp.case(k)
    V, inside, live = ref[:3]
    q, group = quantities(4, 3), stage_groups(cl)
    want_acc, want_tail, want_grp = ir.accumulate(V, inside, q), pr.top_tail(V, inside, T_REF), ir.group_sums(V, inside, group, 2)
    # not vacuous: stated on the reference before the device is consulted
    shift = ir.table(V, inside, q)[:, ir.STAR_HEAD::3]
    moved, wd, sizes = ic.non_vacuity(want_acc, shift, cl, live, group)
    print(f"{name} {n_filt}: {moved} of {n_stars} stars with SNEG > 1 and a shift, {wd} live WD-stage stars, groups {sizes}")
    assert moved >= (9 * n_stars + 9) // 10 and list(inside) == [True, True, True, False]
    if wd_frac > 0:
        assert wd >= 1 and len(sizes) == 2 and sizes.min() >= 1
    eng = make_engine(pack, stars, priors, n_pops, K, Q)
    try:
        got = eng.star_influence(rows, q, T_REF, group, 2)
        eng.set_tuning(marg_no_pruning=1)
        full = eng.star_influence(rows, q, T_REF, group, 2)
        eng.set_tuning()
    finally:
        eng.close()
    for what, (acc, tail, grp) in (("pruned", got), ("unpruned", full)):
        assert acc.shape == (n_stars, 18) and tail.shape == (n_stars, T_REF) and grp.shape == (4, 2)
        ic.assert_acc(acc, want_acc, V, inside, q)
        tp.pc.assert_tail(tail, want_tail)
        ic.assert_groups(grp, want_grp, V, inside, group)
        assert np.all(acc[:, ir.ROWS] == 3) and np.all(acc[:, ir.NINF] == 0)     # the row outside the grid adds nothing to any star
        assert np.all(grp[3] == -np.inf) and np.all(np.isfinite(grp[:3]))


# ---- 2. the reducers in isolation -------------------------------------------------------------------------------------------
def test_reducers_on_the_device_matrix():
    pack_d, cl, pack, stars, priors, _, _ = tp.case(0)
    rows, V, lpd = tp.device_matrix()
    q, group = quantities(40, 3), stage_groups(cl)
    eng = make_engine(pack, stars, priors, 2, 2, 2)
    try:
        acc, _, grp = eng.star_influence(rows, q, 0, group, 2)
    finally:
        eng.close()
    want = ir.accumulate(V, None, q)
    assert np.array_equal(acc[:, :2], want[:, :2]) and np.all(acc[:, ir.ROWS] == 40)
    assert np.array_equal(acc[:, ir.RMAX], (-V).max(axis=0))
    np.testing.assert_allclose(acc, want, rtol=1e-12, atol=0)
    assert np.array_equal(grp, ir.group_sums(V, np.ones(40, bool), group, 2))          # the sequential sum, bit for bit


# ---- 3. ties, bit for bit ---------------------------------------------------------------------------------------------------
def test_ties_to_pointwise():
    pack_d, cl, pack, stars, priors, _, _ = tp.case(0)
    rows = np.array(tp.device_matrix()[0])
    n = len(cl["stage"])
    eng = make_engine(pack, stars, priors, 2, 2, 2)
    try:
        pw_acc, pw_tail, pw_rows = eng.pointwise(rows, 5)
        acc, tail, grp = eng.star_influence(rows, np.ones((40, 2)), 5, np.zeros(n, np.int32), 1)
    finally:
        eng.close()
    assert np.array_equal(acc[:, [ir.ROWS, ir.NINF, ir.RMAX, ir.SNEG]], pw_acc[:, [pr.ROWS, pr.NINF, pr.RMAX, pr.SNEG]])
    assert np.array_equal(tail, pw_tail) and np.array_equal(grp[:, 0], pw_rows)
    assert (acc[:, ir.SNEG] > 1).sum() >= n - 5
    for j in range(2):                                     # q = 1: the weights' own sum
        assert np.array_equal(acc[:, ir.WQ(j)], acc[:, ir.SNEG]) and np.array_equal(acc[:, ir.WQ(j) + 1], acc[:, ir.SNEG])
        assert np.all(acc[:, ir.WQ(j) + 2] == 1.0) and np.all(acc[:, ir.WQ(j) + 3] == 0.0)


# ---- 4. shapes where the kernels can go wrong ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ms,n_wd", [(1, 0), (1, 1), (1, 4), (1, 5), (64, 1), (65, 1), (255, 1), (256, 1), (257, 1)])
def test_star_count_edges(n_ms, n_wd):
    pack_d, cl, pack, _, priors, _ = build_problem("parsec", 4, n_stars=400, wd_frac=0.1, seed=12)
    stage = np.asarray(cl["stage"])
    ms, wd = np.flatnonzero(stage != abi.STAGE_WD)[:n_ms], np.flatnonzero(stage == abi.STAGE_WD)[:n_wd]
    assert len(ms) == n_ms and len(wd) == n_wd
    cl = tm.subset(cl, np.sort(np.concatenate([ms, wd])))
    rows = tm.rows_for(pack_d, cl, 1, 2)
    V, inside, _ = pr.v_matrix(pack_d, cl, rows, 1, 2, 2)
    q, group = quantities(len(rows), 3), stage_groups(cl)
    eng = make_engine(pack, abi.make_stars(cl), priors, 1, 2, 2)
    try:
        acc, tail, grp = eng.star_influence(rows, q, T_REF, group, 2)
    finally:
        eng.close()
    ic.assert_acc(acc, ir.accumulate(V, inside, q), V, inside, q)
    tp.pc.assert_tail(tail, pr.top_tail(V, inside, T_REF))
    ic.assert_groups(grp, ir.group_sums(V, inside, group, 2), V, inside, group)
    assert np.all(acc[:, ir.ROWS] == 2)


@functools.lru_cache(maxsize=None)
def matrix65():
    """The small pack, 65 rows about the truth, and the device's own v matrix from 65 single-row b9_pointwise calls."""
    pack_d, cl, pack, stars, priors, _ = tp.small()
    rows = synth.walker_params(cl["truth"], 65, seed=8, scale=0.3)
    eng = make_engine(pack, stars, priors, 1, 2, 2)
    try:
        V = np.empty((65, eng.n_stars))
        for r in range(65):
            acc, _, _ = eng.pointwise(rows[r:r + 1], want_rows=False)
            assert np.all(acc[:, pr.ROWS] == 1) and np.all(acc[:, pr.NINF] == 0)
            V[r] = acc[:, pr.VMAX]
    finally:
        eng.close()
    rows.setflags(write=False); V.setflags(write=False)
    return rows, V


@pytest.mark.parametrize("n_rows", [1, 31, 32, 33, 65])
def test_row_count_edges(n_rows):
    pack_d, cl, pack, stars, priors, _ = tp.small()
    rows, V = matrix65()
    q, group = quantities(65, 3)[:n_rows], stage_groups(cl)
    eng = make_engine(pack, stars, priors, 1, 2, 2)
    try:
        acc, tail, grp = eng.star_influence(rows[:n_rows], q, 3, group, 2)
    finally:
        eng.close()
    want = ir.accumulate(V[:n_rows], None, q)
    assert np.array_equal(acc[:, :3], want[:, :3]) and np.all(acc[:, ir.ROWS] == n_rows)
    np.testing.assert_allclose(acc, want, rtol=1e-12, atol=0)
    assert np.array_equal(tail, pr.top_tail(V[:n_rows], np.ones(n_rows, bool), 3))
    assert np.array_equal(grp, ir.group_sums(V[:n_rows], np.ones(n_rows, bool), group, 2))


def test_quantity_count_edges():
    """Q = 1, 2, 3, 4, 5, 8, 9 and 12: one tile of 1, of 2, of 4 (one partial), two and three tiles (the last partial or whole).  A
    quantity's four columns are the Q = 1 call's, wherever it stands."""
    pack_d, cl, pack, stars, priors, _ = tp.small()
    rows = np.array(matrix65()[0][:33])
    q = quantities(33, 12)
    eng = make_engine(pack, stars, priors, 1, 2, 2)
    try:
        alone = [eng.star_influence(rows, q[:, j:j + 1])[0] for j in range(12)]
        for Q in (1, 2, 3, 4, 5, 8, 9, 12):
            for cols in (np.arange(Q), np.arange(12)[::-1][:Q]):
                acc = eng.star_influence(rows, q[:, cols])[0]
                assert acc.shape == (eng.n_stars, 6 + 4 * Q)
                for p, j in enumerate(cols):
                    assert np.array_equal(acc[:, :6], alone[j][:, :6]) and np.array_equal(acc[:, ir.WQ(p):ir.WQ(p) + 4], alone[j][:, 6:]), (Q, p, j)
    finally:
        eng.close()
    assert all((a[:, ir.WQ(0) + 3] != 0).sum() >= 60 for a in alone)


def test_group_count_edges():
    """G = 1, 2 and 8, stars with id -1 among them: a group's sums are the group-alone call's."""
    pack_d, cl, pack, stars, priors, _ = tp.small()
    rows = np.array(matrix65()[0][:5])
    rng = np.random.default_rng(3)
    eng = make_engine(pack, stars, priors, 1, 2, 2)
    try:
        n = eng.n_stars
        for G in (1, 2, 8):
            group = rng.integers(-1, G, n).astype(np.int32)
            group[0], group[1] = -1, G - 1
            grp = eng.star_influence(rows, groups=group, n_groups=G)[2]
            assert grp.shape == (5, G) and np.all(np.isfinite(grp))
            for g in range(G):
                one = eng.star_influence(rows, groups=np.where(group == g, 0, -1).astype(np.int32), n_groups=1)[2]
                assert np.array_equal(one[:, 0], grp[:, g]), (G, g)
            assert np.array_equal(eng.star_influence(rows, groups=np.full(n, -1, np.int32), n_groups=G)[2], np.zeros((5, G)))      # empty groups
    finally:
        eng.close()


# ---- 5. bitwise invariances -------------------------------------------------------------------------------------------------
def test_bitwise_invariances():
    pack_d, cl, pack, stars, priors, _ = tp.small()
    rows = np.array(matrix65()[0])
    q, group, T = quantities(65, 5), stage_groups(cl), 5
    eng = make_engine(pack, stars, priors, 1, 2, 2)
    try:
        whole = eng.star_influence(rows, q, T, group, 2)
        assert np.all(whole[0][:, ir.ROWS] == 65) and (whole[0][:, ir.SNEG] > 1).sum() >= 60
        for k in (1, 2, 3):                                # every split of the 65 rows at 1, 32 and 33
            for cuts in itertools.combinations((1, 32, 33), k):
                state, grp = None, []
                for a, b in zip((0,) + cuts, cuts + (65,)):
                    acc, tail, g = eng.star_influence(rows[a:b], q[a:b], T, group, 2, state)
                    state = (acc, tail)
                    grp.append(g)
                assert same((acc, tail, np.concatenate(grp)), whole), cuts
        # acc alone, the groups alone
        only = eng.star_influence(rows, q, 0)
        assert only[1] is None and only[2] is None and np.array_equal(only[0], whole[0])
        assert np.array_equal(eng.star_influence(rows, groups=group, n_groups=2)[2], whole[2])
        # a row outside the grid in the middle of a batch changes nothing but its own sums
        outside = rows[:1].copy(); outside[0, abi.P_LOGAGE] = pack_d["log_age"][-1] + 1.0
        mixed = eng.star_influence(np.concatenate([rows[:7], outside, rows[7:]]), np.concatenate([q[:7], q[:1], q[7:]]), T, group, 2)
        assert np.array_equal(mixed[0], whole[0]) and np.array_equal(mixed[1], whole[1])
        assert np.all(mixed[2][7] == -np.inf) and np.array_equal(np.delete(mixed[2], 7, axis=0), whole[2])
        # a repeated call on a long-lived engine; the siblings in between leave nothing behind
        eng.star_moments(rows[:7]); eng.pointwise(rows[:5], 3)
        assert same(eng.star_influence(rows, q, T, group, 2), whole)
    finally:
        eng.close()
    eng = make_engine(pack, stars, priors, 1, 2, 2)                           # a fresh context
    try:
        assert same(eng.star_influence(rows, q, T, group, 2), whole)
    finally:
        eng.close()


def test_scratch_rule_picks_the_chunk():
    """70000 stars: a row's values take 560 kB, so the 16 MiB rule allows 29 rows a chunk (test_gpu_pointwise's case).  33 rows in
    one call (29 + 4) = 16 + 17 continued."""
    pack_d, cl, pack, stars, priors, _ = build_problem("parsec", 4, n_stars=70000, wd_frac=0.02, seed=12)
    assert (16 << 20) // (8 * 70000) == 29
    rows = synth.walker_params(cl["truth"], 33, seed=8, scale=0.3)
    q, group = quantities(33, 5), stage_groups(cl)
    eng = make_engine(pack, stars, priors, 1, 1, 2)
    try:
        whole = eng.star_influence(rows, q, 3, group, 2)
        acc, tail, g0 = eng.star_influence(rows[:16], q[:16], 3, group, 2)
        acc, tail, g1 = eng.star_influence(rows[16:], q[16:], 3, group, 2, (acc, tail))
        v0 = eng.pointwise(rows[:1], want_rows=False)[0][:, pr.VMAX]
    finally:
        eng.close()
    # 136 batches of 512 stars, five of 64 and one of 48: the groups' sums are still the sequential ones, bit for bit
    assert np.array_equal(whole[2][:1], ir.group_sums(v0[None, :], np.ones(1, bool), group, 2))
    assert np.all(whole[0][:, ir.ROWS] == 33) and (whole[0][:, ir.SNEG] > 1).sum() >= 60000
    assert same((acc, tail, np.concatenate([g0, g1])), whole)


def test_quantity_tiles_on_a_large_catalogue():
    """70000 stars, Q = 12 and Q = 5: three and two tiles of 274 workgroups each, more workgroups than the device holds at once at
    Q = 12 (three 256-lane workgroups per SIMD at 132 registers: 768).  No tile may read a head that another has already
    advanced: every quantity's columns, and the head, are the Q = 1 call's, over two continued calls (the second finds k > 0)."""
    pack_d, cl, pack, stars, priors, _ = build_problem("parsec", 4, n_stars=70000, wd_frac=0.02, seed=12)
    rows = synth.walker_params(cl["truth"], 6, seed=8, scale=0.3)
    q = quantities(6, 12)
    eng = make_engine(pack, stars, priors, 1, 1, 2)

    def two_calls(qq):
        acc, _, _ = eng.star_influence(rows[:3], qq[:3])
        return eng.star_influence(rows[3:], qq[3:], state=(acc, None))[0]

    try:
        alone = [two_calls(q[:, j:j + 1]) for j in range(12)]
        for Q in (5, 12):
            acc = two_calls(q[:, :Q])
            assert np.all(acc[:, ir.ROWS] == 6) and (acc[:, ir.SNEG] > 1).sum() >= 60000
            for j in range(Q):
                assert np.array_equal(acc[:, :6], alone[j][:, :6]) and np.array_equal(acc[:, ir.WQ(j):ir.WQ(j) + 4], alone[j][:, 6:]), (Q, j)
    finally:
        eng.close()
    assert all((a[:, ir.WQ(0) + 3] != 0).sum() >= 60000 for a in alone)


# ---- 6. a star with v = -inf in one row -----------------------------------------------------------------------------------------
def test_a_row_that_gives_a_star_no_likelihood():
    """test_gpu_pointwise's case: a parametrised IFMR that gives M_wd <= 0 at every node in row 1, a WD-stage star at membership
    prior 1: its NINF, the untouched rest of its state, and its group's -inf."""
    pack_d, cl, pack, _, priors, _ = build_problem("parsec", 4, n_stars=70, wd_frac=0.1, seed=12, ifmr_id=abi.IFMR_LINEAR)
    cl = tm.subset(cl, np.arange(70))
    cl["clust_prior"] = np.array(cl["clust_prior"], dtype=np.float64)
    one = np.flatnonzero(np.asarray(cl["stage"]) == abi.STAGE_WD)[1]
    cl["clust_prior"][one] = 1.0
    rows = np.array(tm.rows_for(pack_d, cl, 1, 3, outside=False))
    rows[1, abi.P_IFMR_INTERCEPT], rows[1, abi.P_IFMR_SLOPE] = -10.0, 0.0
    V, inside, _ = pr.v_matrix(pack_d, cl, rows, 1, 2, 2)
    assert inside.all() and V[1, one] == -np.inf and np.isfinite(np.delete(V, one, axis=1)).all()
    q, group = quantities(3, 2), stage_groups(cl)
    eng = make_engine(pack, abi.make_stars(cl), priors, 1, 2, 2)
    try:
        a0, t0, g0 = eng.star_influence(rows[0:1], q[0:1], 2, group, 2)
        a01, t01, g01 = eng.star_influence(rows[1:2], q[1:2], 2, group, 2, (a0, t0))
        whole = eng.star_influence(rows, q, 2, group, 2)
    finally:
        eng.close()
    assert a0[one, ir.ROWS] == 1 and a0[one, ir.NINF] == 0
    assert a01[one, ir.ROWS] == 2 and a01[one, ir.NINF] == 1 and np.array_equal(a01[one, ir.RMAX:], a0[one, ir.RMAX:]) and np.array_equal(t01[one], t0[one])
    assert g01[0, 1] == -np.inf and np.isfinite(g01[0, 0]) and np.all(np.isfinite(g0))
    assert whole[0][one, ir.NINF] == 1 and np.all(np.delete(whole[0][:, ir.NINF], one) == 0)
    ic.assert_acc(whole[0], ir.accumulate(V, inside, q), V, inside, q)
    ic.assert_groups(whole[2], ir.group_sums(V, inside, group, 2), V, inside, group)


# ---- 7. leaves the sampler alone --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [abi.MODE_GIVEN_MASS, abi.MODE_MARGINALISED])
def test_sampler_blocks_are_untouched(mode):
    from base_amd import mcmc
    pack_d, cl, pack, stars, priors, _, _ = tp.case(1)
    free = np.array(mcmc.DEFAULT_FREE)
    chol = np.diag([mcmc.DEFAULT_STEP[k] for k in free]) * 0.3
    start = synth.walker_params(cl["truth"], 4, seed=2, scale=0.3)
    rows = tm.rows_for(pack_d, cl, 1)
    q, group = quantities(len(rows), 2), stage_groups(cl)

    def run(interleave):
        eng = make_engine(pack, stars, priors, 1, 1, 4, mode)
        try:
            lp0 = eng.logpost(start)
            h = eng.mcmc_submit(start, lp0, np.arange(4), free, chol, 11, 0, 6, asynchronous=True)
            if interleave:
                with pytest.raises(Exception) as e:                        # B9_ERR_STATE: a block is outstanding
                    eng.star_influence(rows, q, 2, group, 2)
                assert e.value.code == abi.B9_ERR_STATE and "outstanding" in str(e.value)
            first = [np.array(x) for x in eng.mcmc_collect(h)[:4]]
            if interleave:
                acc, _, _ = eng.star_influence(rows, q, 2, group, 2)
                assert np.all(acc[:, ir.ROWS] == 3)
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
    pack_d, cl, pack, stars, priors, rows = tp.small()
    eng = make_engine(pack, stars, priors, 1, 2, 2)
    try:
        n = eng.n_stars
        rows = np.ascontiguousarray(rows)

        def call(n_rows=4, acc=True, tail=True, grp=True, params=True, ctx=True, tail_len=3, n_q=2, q=True, bad_q=None, n_groups=2, group=True, bad_id=None):
            a, t, g = np.full((n, 6 + 4 * 12), 7.25), np.full((n, 256), 7.25), np.full((4, 8), 7.25)
            qq, ids = np.ones((4, max(n_q, 2))), np.zeros(n, np.int32)
            if bad_q is not None:
                qq[2, 1] = bad_q
            if bad_id is not None:
                ids[n - 1] = bad_id
            code = eng.lib.b9_star_influence(eng._ctx if ctx else None, rows.ctypes.data_as(_dp) if params else None, n_rows, 0, n_q,
                                             qq.ctypes.data_as(_dp) if q else None, a.ctypes.data_as(_dp) if acc else None, tail_len,
                                             t.ctypes.data_as(_dp) if tail else None, n_groups, ids.ctypes.data_as(_ip) if group else None,
                                             g.ctypes.data_as(_dp) if grp else None)
            assert code == abi.B9_OK or (np.all(a == 7.25) and np.all(t == 7.25) and np.all(g == 7.25))
            return code

        assert call() == abi.B9_OK
        assert call(n_rows=0) == abi.B9_ERR_INVALID and call(n_rows=-2) == abi.B9_ERR_INVALID
        assert call(params=False) == abi.B9_ERR_INVALID and call(ctx=False) == abi.B9_ERR_INVALID
        assert call(acc=False, tail=False, grp=False) == abi.B9_ERR_INVALID
        assert call(n_q=0) == abi.B9_ERR_INVALID and call(n_q=13) == abi.B9_ERR_INVALID and call(q=False) == abi.B9_ERR_INVALID
        assert call(bad_q=np.nan) == abi.B9_ERR_INVALID and call(bad_q=np.inf) == abi.B9_ERR_INVALID
        assert call(tail_len=-1) == abi.B9_ERR_INVALID and call(tail_len=257) == abi.B9_ERR_INVALID
        assert call(acc=False) == abi.B9_ERR_INVALID                       # tail without acc
        assert call(n_groups=0) == abi.B9_ERR_INVALID and call(n_groups=9) == abi.B9_ERR_INVALID and call(group=False) == abi.B9_ERR_INVALID
        assert call(bad_id=2) == abi.B9_ERR_INVALID and call(bad_id=-2) == abi.B9_ERR_INVALID
        assert call(tail_len=256) == abi.B9_OK and call(tail_len=0) == abi.B9_OK and call(n_q=12, n_groups=8, bad_id=7) == abi.B9_OK
        assert call(acc=False, tail=False, n_q=0, q=False) == abi.B9_OK and call(grp=False, n_groups=0, group=False) == abi.B9_OK
        assert call(tail=False) == abi.B9_OK and call(bad_id=-1) == abi.B9_OK
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
def test_a_displaced_turn_off_star_drives_the_age():
    """A 130-star single-population catalogue, 64 rows spread about the truth, q = the z-score of logAge.  The turn-off star (the
    MS/RGB-stage star of largest primary mass) is moved 0.3 mag brighter in every filter: the reference says that it then ranks
    first in |lin| for logAge, and that it did not before (seed 13: the star is an unequal binary, so the move leaves it a
    member; a single star 0.3 mag off the locus falls to the field term, whose v does not vary and which moves nothing).  The
    device's state through the host table gives the same ranking."""
    from base_amd import hostlib
    pack_d, cl, pack, _, priors, _ = build_problem("parsec", 4, n_stars=130, wd_frac=0.1, seed=13)
    cl = tm.subset(cl, np.arange(130))
    ms = np.flatnonzero(np.asarray(cl["stage"]) == abi.STAGE_MSRG)
    star = int(ms[np.argmax(np.asarray(cl["mass1"])[ms])])
    rows = synth.walker_params(cl["truth"], 64, seed=8, scale=0.3)
    q = ir.zscores(rows[:, [abi.P_LOGAGE]])[0]
    V0, inside, _ = pr.v_matrix(pack_d, cl, rows, 1, 2, 2)
    cl["obs"] = np.array(cl["obs"], dtype=np.float64)
    cl["obs"][star] -= 0.3
    V = V0.copy()
    V[:, star] = pr.v_matrix(pack_d, tm.subset(cl, np.array([star])), rows, 1, 2, 2)[0][:, 0]
    assert inside.all()
    before, want = ir.table(V0, inside, q), ir.table(V, inside, q)
    lin0, lin = np.abs(before[:, ir.STAR_HEAD + 1]), np.abs(want[:, ir.STAR_HEAD + 1])
    print(f"reference: star {star}: |lin| {lin0[star]:.3f} (rank {int((lin0 > lin0[star]).sum())}) -> {lin[star]:.3f}, the next {np.sort(lin)[-2]:.3f}")
    assert np.argmax(lin) == star and np.argmax(lin0) != star and lin[star] > 1.2 * np.sort(lin)[-2]
    eng = make_engine(pack, abi.make_stars(cl), priors, 1, 2, 2)
    try:
        acc, _, _ = eng.star_influence(rows, q)
    finally:
        eng.close()
    ic.assert_acc(acc, ir.accumulate(V, inside, q), V, inside, q)
    got = hostlib.influence_table(acc)
    assert np.argmax(np.abs(got[:, ir.STAR_HEAD + 1])) == star
    want[:, 3] = np.nan                                  # (no tail was kept: no fit)
    ic.assert_table(got, want, V, inside, q)


# ---- 10. the CLI --------------------------------------------------------------------------------------------------------------
def test_cli_star_influence(tmp_path):
    """simCluster (200 stars) -> scatterCluster -> singlePopMcmc (short, 4 walkers x 100 main-run rows: the program passes them in
    two batches, the second continued) -> starInfluence: the three files parse and equal what Engine.star_influence in ONE call
    gives through the host tables, with the quantities and the groups the host library forms from the same rows."""
    import math
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
    r = _cli("starInfluence", "--config", y)
    assert r.returncode == 0, r.stderr
    assert "star rows/s" in r.stderr and "shift without the star" in r.stdout and "without group ms" in r.stdout

    cl = tm._read_phot(base + ".sim.scatter")
    phot_ids = [ln.split()[0] for ln in open(base + ".sim.scatter").read().splitlines()[1:]]
    rows = hostlib.read_res_rows(fit + ".res", start, 3)
    S = len(rows)
    assert S == 100 * 4                                   # more than one batch of 256
    T = min(256, min(S // 5, math.ceil(3 * math.sqrt(S))) + 1)
    names, q, mean, sd = hostlib.influence_quantities([], rows)
    gnames, group = hostlib.influence_groups([], phot_ids, cl["stage"])
    assert len(names) >= 3 and gnames == ["ms", "wd"] and (group == 0).sum() >= 100
    eng = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cl), synth.default_priors(pack_d, truth), tm.opts(1, K, Q))
    try:
        acc, tail, grp = eng.star_influence(rows, q, T, group, 2)
    finally:
        eng.close()
    ids, cols, tab = hostlib.read_star_influence(fit + ".starInfluence")
    assert ids == phot_ids and cols[:4] == list(hostlib.INFLUENCE_HEAD) and cols[4:7] == [f"{w}_{names[0]}" for w in ("shift", "lin", "looSd")]
    assert np.array_equal(tab, hostlib.influence_table(acc, tail), equal_nan=True)
    assert np.all(tab[:, 0] == S) and np.all(tab[:, 1] == 0) and np.isfinite(tab[:, 3]).sum() >= 150 and (tab[:, 4] != 0).sum() >= 150
    gids, gcols, gtab = hostlib.read_group_influence(fit + ".groupInfluence")
    assert gids == gnames and gcols[:5] == list(hostlib.GROUP_INFLUENCE_HEAD)
    assert np.array_equal(gtab, hostlib.group_influence_table(grp, q, group), equal_nan=True)
    snames, scols, scale = hostlib.read_influence_scale(fit + ".influenceScale")
    assert snames == names and scols == ["mean", "sd"] and np.array_equal(scale[:, 0], mean) and np.array_equal(scale[:, 1], sd)
    # named quantities, no groups: the named columns are the default run's
    r = _cli("starInfluence", "--config", y, "--quantity", names[1], "--quantity", "logPost", "--noGroups", "--outputFileBase", fit)
    assert r.returncode == 0, r.stderr
    _, cols2, tab2 = hostlib.read_star_influence(fit + ".starInfluence")
    assert cols2[4] == "shift_" + names[1] and cols2[7] == "shift_logPost" and np.array_equal(tab2[:, 4:7], tab[:, 7:10], equal_nan=True)
