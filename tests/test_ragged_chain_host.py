"""The ragged saved-chain scripts (tests/ragged_chain.py) on the CPU: what the scripts must reach for the GPU comparison in
tests/test_gpu_ragged_chain.py to test anything, asserted from the restatements of tests/ragged_walk.py; that the comparison is
not vacuous and is well conditioned, stated on the references alone; and the comparators' own power: seven faulty stand-ins,
applied to the references' nodes, must be rejected by every comparator they can affect, at the families' own tolerances.

The conditions are properties of the inputs (pack, catalogue, scripts), not of the code under test: an input that misses one is
replaced here, on the CPU."""
import collections
import contextlib
import io
import os

import numpy as np
import pytest

import moments_ref as mr
import pointwise_check as pc
import ragged_chain as rcn
import ragged_walk as rw
import resid_check as rc
import test_gpu_moments as tm
import wdmoments_check as wc
import wdmoments_ref as wr
from base_amd import abi

COMBO_IDS = [f"{s}-k{K}q{Q}" for s, K, Q in rcn.COMBOS]


def quiet(check, *args, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return rcn.rejects(check, *args, **kw)


# ---- what the scripts reach ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", list(rcn.SETTINGS))
def test_the_scripts_reach_every_transition_on_both_sides_of_the_seam(setting):
    prob = rcn.problem(setting)
    pack_d, n_pops = prob["pack_d"], prob["n_pops"]
    assert prob["n_stars"] <= 200 and all(34 <= len(r) <= 40 for r in prob["scripts"])
    # every call's chunk -- b9_pointwise's own cap and scratch rule included -- holds rcn.CHUNK rows at these sizes
    assert set(rcn.chunk_rows_of_the_calls(prob["n_stars"], pack_d["n_filt"]).values()) == {rcn.CHUNK}
    # the WD family has drivers and a chunk rule of its own (256 rows, 64 MiB of node tables): at 63 and 65 nodes a whole script is
    # ONE chunk, so rows 31 | 32 are no seam of theirs; at wd_seam_nodes the table rule cuts chunks of 32 rows and they are
    n_wd, longest = len(prob["wd"]), max(len(r) for r in prob["scripts"])
    for call in rcn.WD_FAMILY:
        for n_nodes in rcn.WD_NODES:
            assert rcn.wd_family_chunk(call, longest, pack_d["n_filt"], n_pops, n_nodes, n_wd, rcn.WD_BINS) == longest
        seam = rcn.wd_seam_nodes(call, pack_d["n_filt"], n_pops, n_wd, rcn.WD_BINS)
        assert rcn.wd_family_chunk(call, longest, pack_d["n_filt"], n_pops, seam, n_wd, rcn.WD_BINS) == rcn.CHUNK
        assert rcn.wd_family_chunk(call, longest, pack_d["n_filt"], n_pops, seam // 2, n_wd, rcn.WD_BINS) > rcn.CHUNK
    for K in (1, 2, 3):
        total = collections.Counter()
        for rows in prob["scripts"]:
            total.update(rcn.script_tags(pack_d, rows, K, n_pops))
        missing = [f"{t}@{s}" for t in rcn.TRANSITIONS for s in rcn.SIDES if not total[f"{t}@{s}"]]
        assert not missing, (K, missing)
        # (n - 1) K just below, on and just above a multiple of 64
        assert total["mod0"] and total[f"mod{64 - K}"] and total[f"mod{K}"], (K, sorted(t for t in total if t.startswith("mod")))
        chunks = {rcn.row_facts(pack_d, r, K, n_pops)[2] for rows in prob["scripts"] for r in rows}
        assert chunks >= {1: {0, 1, 2, 3}, 2: {0, 1, 2, 3, 5}, 3: {0, 1, 2, 3, 4, 8}}[K], (K, chunks)
    # the one-interval row directly after (and before) a row of five chunks: K = 2
    facts = [[rcn.row_facts(pack_d, r, 2, n_pops) for r in rows] for rows in prob["scripts"]]
    assert any(a[2] == 5 and b[1] == 2 for f in facts for a, b in zip(f, f[1:])) and any(a[1] == 2 and b[2] == 5 for f in facts for a, b in zip(f, f[1:]))


def test_the_seam_transitions_sit_on_rows_31_and_32():
    prob = rcn.problem("base4")
    for k, rows in enumerate(prob["scripts"]):
        a, b = (rcn.row_facts(prob["pack_d"], rows[j], 2, 1) for j in (31, 32))
        want = [("outside", 0) if t == rcn.OUT else (("invalid", 0) if t == rcn.INVALID_CELL else ("valid", rw.LADDER_COMMON[t])) for t in rcn.SEAMS[k]]
        assert [a[:2], b[:2]] == want, k


def test_the_record_of_the_cases_is_current():
    path = os.path.join(abi.REPO_ROOT, "profiles", "ragged_chain_cases.md")
    assert open(path).read().strip() == rcn.cases_markdown().strip(), "regenerate with: PYTHONPATH=.:tests python tests/ragged_chain.py > profiles/ragged_chain_cases.md"


# ---- non-vacuity, on the reference alone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting,K,Q", rcn.COMBOS, ids=COMBO_IDS)
def test_every_rung_class_has_stars_that_test_something(setting, K, Q):
    ref = rcn.reference(setting, K, Q)
    prob = ref.prob
    pack_d, cl, n_pops = prob["pack_d"], prob["cl"], prob["n_pops"]
    ms = np.asarray(cl["stage"]) != abi.STAGE_WD
    assert (~ms).sum() >= 15
    for name, cells in rcn.RUNGS.items():
        rows = np.stack([r for r in ref.distinct if rw.cell_of(pack_d, r)[0][0] in cells and not rw.cell_of(pack_d, r)[1]])
        assert len(rows) >= 3
        x = ref.moments(rows)
        assert np.all(x[:, :, mr.ROWS] == 1), "every valid row counts every star"
        tab = np.stack([mr.table(xr) for xr in x])
        member = ms[None, :] & (tab[:, :, 1] > 1e-3)
        # a table of one node (one interval at K = 1) gives every star the same mass: no spread to ask for
        spread = member & (tab[:, :, 3] > 1e-6) if (rw.LADDER_COMMON[cells[0]] - 1) * K > 1 else member
        binary = spread & (tab[:, :, 6] > 0.01) & (tab[:, :, 6] < 0.99)
        print(f"{name}: per row, MS-stage stars with membership > 1e-3 and mass sd > 1e-6: {spread.sum(axis=1)}; with P(binary) inside: {binary.sum(axis=1)}")
        assert spread.sum(axis=1).max() >= 8 and binary.sum(axis=1).max() >= 4
        tip = max(rw.mass_column(pack_d, rows[0], p)[-1] for p in range(n_pops))
        assert tip < pack_d["m_wd_up"]
        for n_nodes in rcn.WD_NODES:
            xw = ref.wd_moments(n_nodes, rows)[0]
            live = (xw[:, :, wr.MEMBER] > 0) & (xw[:, :, wr.M1] > 0)
            assert np.all(xw[:, :, wr.ROWS] == 1) and live.sum(axis=1).min() >= 3, (name, n_nodes, live.sum(axis=1))
            # (test_gpu_wdmass.check_derived leaves no draw out: an error in the precursor's age is amplified less than A_MAX times)
            assert ref.wd_moments(n_nodes, rows)[2].max() <= wc.A_MAX
    none = [r for r in ref.distinct if rcn.row_facts(pack_d, r, K, n_pops)[0] != "valid"]
    kinds = {rcn.row_facts(pack_d, r, K, n_pops)[0] for r in none}
    assert kinds == {"invalid", "outside"}
    assert np.all(ref.moments(np.stack(none)) == 0) and np.all(ref.wd_moments(rcn.WD_NODES[0], np.stack(none))[0] == 0), "a row without isochrone counts no star"
    V, inside, _ = ref.pointwise(np.stack(none))
    assert not inside.any()


# ---- conditioning: the fp64 references against their node terms in longdouble ----------------------------------------------------
@pytest.mark.parametrize("setting,K,Q", rcn.COMBOS, ids=COMBO_IDS)
def test_the_references_are_well_conditioned(setting, K, Q):
    """Every sum the moment, binned and residual calls compare is a sum of membership-weighted node weights p w (times exact
    factors); b9_pointwise compares v.  With the node terms evaluated again in np.longdouble, every p w of every (distinct row,
    star) of the scripts stays within a tenth of the families' tolerance -- rtol (test_gpu_moments.RTOL, the same 1e-9 in
    masshist_check, resid_check, wdmoments_check) plus the e^-40 (resid_check.CUT) below which the families' absolute term
    takes over -- and v within a tenth of pointwise_check.TOL max(1, |v|).  The WD-stage stars are in it on all three grids: the
    8 K steps of the chain_reduce calls and the b9_wd_* calls' 63 and 65 nodes.  The bound on p w is built from the families'
    constants; it stands in for their comparators (whose entries are sums of such p w times exact factors), it is not one of them."""
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is no wider than double here"
    assert tm.RTOL == rc.RTOL == wc.RTOL
    ref = rcn.reference(setting, K, Q)
    prob = ref.prob
    cl, wd = prob["cl"], prob["wd"]
    worst_w = worst_v = 0.0
    wn = [ref.wd_nodes(n, ref.distinct) for n in rcn.WD_NODES]
    for r, (par, nodes) in enumerate(zip(ref.distinct, ref.nodes(ref.distinct))):
        if nodes is None:
            continue
        empty = (np.empty(0), np.empty(0), np.empty(0), np.empty(0, int))
        grids = [(nodes, None)]
        for n, per_row in zip(rcn.WD_NODES, wn):
            as_ms = [empty] * prob["n_stars"]
            for c, i in enumerate(wd):
                t, m, k, _, _ = per_row[r][c]
                as_ms[i] = (t, m, np.zeros(len(t)), k)
            grids.append((as_ms, n))
        for grid, steps in grids:
            wide = rcn.terms_longdouble(prob, K, Q, par, grid, wd_steps=steps)
            for i, nd in enumerate(grid):
                if len(nd[0]) == 0:
                    continue
                pw, v = rcn.node_weights(cl, i, nd[0])
                pw_wide, v_wide = rcn.node_weights(cl, i, wide[i])
                worst_w = max(worst_w, float(np.max(np.abs(pw - pw_wide) / (tm.RTOL * np.abs(pw_wide) + rc.CUT))))
                worst_v = max(worst_v, float(abs(v - v_wide) / (pc.TOL * max(1.0, abs(v_wide)))))
    print(f"largest departure of the fp64 reference from longdouble, in tolerances: node weights {worst_w:.3g}, v {worst_v:.3g}")
    assert worst_w <= 0.1 and worst_v <= 0.1


# ---- the comparators' power ------------------------------------------------------------------------------------------------------
#: the calls a stand-in can affect.  seed_reads_past_end raises the walk's bound: what it drops weighs less than e^-40 of the
#: stale term, and a stale term that far above a star's largest makes a star without membership -- so it shows only where a star
#: loses every node and with them its row COUNT, which b9_star_moments and b9_phot_resid keep per star (tests/ragged_chain.py).
AFFECTED = {k: rcn.MS_CALLS for k in rcn.AFFECTS_MS}
AFFECTED["seed_reads_past_end"] = ("star_moments", "phot_resid")
AFFECTED["stale_tip"] = rcn.MS_CALLS
#: (setting, K, Q, scripts): the seams of scripts 0 (158 -> 2 points), 3 (66 -> 65) and 8 (158 -> 66) are those at which a row that
#: opens a chunk is shorter than the row before it.  At K = 1 script 3's seam leaves ONE surplus node, the heaviest of the row
#: before: b9_mass_hist's bins (shared by all stars) cannot tell it from the row's own heaviest node, the other four calls can;
#: script 8 crosses the seam with 92 surplus nodes instead.
POWER = [("base4", 2, 2, (0, 3)), ("wdragged5", 3, 2, (0,)), ("base9", 1, 2, (0, 8))]


@pytest.mark.parametrize("kind", rcn.STAND_INS)
@pytest.mark.parametrize("setting,K,Q,scripts", POWER, ids=[f"{s}-k{K}q{Q}" for s, K, Q, _ in POWER])
def test_a_faulty_stand_in_is_rejected_by_every_comparator_it_can_affect(setting, K, Q, scripts, kind):
    ref = rcn.reference(setting, K, Q)
    prob = ref.prob
    for k in scripts:
        rows = prob["scripts"][k]
        honest = rcn.ms_outputs(ref, rows)
        r2, n2 = rcn.stand_in_ms(kind, prob, K, Q, rows, ref.nodes(rows))
        faulty = rcn.ms_outputs(ref, r2, n2, honest_rows=rows)
        for call in rcn.MS_CALLS:
            assert not quiet(rcn.check_call, call, honest[call][0], honest[call][1], ref), (call, "the honest reference is rejected")
            if call in AFFECTED[kind]:
                assert quiet(rcn.check_call, call, faulty[call][0], honest[call][1], ref), (kind, call, k)
        if kind in rcn.AFFECTS_WD_FAMILY:
            n_nodes = rcn.WD_NODES[k % 2]
            honest = rcn.wd_outputs(ref, n_nodes, rows)
            r2, n2 = rcn.stand_in_wd(kind, prob, n_nodes, rows, ref.wd_nodes(n_nodes, rows))
            faulty = rcn.wd_outputs(ref, n_nodes, r2, n2)
            for call in rcn.WD_CALLS:
                assert not quiet(rcn.check_call, call, honest[call][0], honest[call][1], ref)
                assert quiet(rcn.check_call, call, faulty[call][0], honest[call][1], ref), (kind, call, k)
            # b9_sample_wd_mass's comparator, on numpy draws from the nodes (ragged_chain.wd_sample_outputs): the honest ones pass
            # -- membership, the count of draws, the row's own grid and test_gpu_wdmass.check_derived's derived values --, the
            # stand-in's do not
            xm = honest["wd_moments"][1]
            draws = rcn.wd_sample_outputs(prob, rows, ref.wd_nodes(n_nodes, rows), seed=k)
            assert not quiet(rcn.check_wd_sample, draws, xm, prob, rows, n_nodes)
            assert quiet(rcn.check_wd_sample, rcn.wd_sample_outputs(prob, r2, n2, seed=k), xm, prob, rows, n_nodes), (kind, "sample_wd_mass", k)


def test_the_binned_calls_edges_keep_clear_of_the_nodes():
    """b9_wd_bins' edges lie at least wdbins_check.MARGIN tolerances from every node value of their line (the device's value of a
    node may differ from the reference's by that tolerance); nine in ten stars' own edges of b9_star_bins straddle their masses:
    three or more inner bins with weight, and weight below the first edge and above the last."""
    import starbins_check as sc
    import wdbins_check as bc
    for setting, K, Q in (("base4", 2, 2), ("wdragged5", 1, 2)):
        ref = rcn.reference(setting, K, Q)
        for n_nodes in rcn.WD_NODES:
            assert ref.wd_edges(n_nodes)[1] >= bc.MARGIN
        acc = rcn.summed(ref.bins(ref.distinct))
        inner, C = sc.bins_with_mass(acc)
        assert (inner[C > 0] >= 3).mean() >= 0.9 and (acc[C > 0, 0] > 0).mean() >= 0.9 and (acc[C > 0, rcn.STAR_BINS + 1] > 0).mean() >= 0.9


@pytest.mark.parametrize("setting", list(rcn.SETTINGS))
def test_the_cooled_nodes_of_a_wd_stage_star_carry_weight(setting):
    """b9_wd_moments' derived columns are compared on the scale p sum_cooled w |v| of the reference (wdmoments_check's floor).
    Where every cooled node of a star lay some 700 e-folds below its largest term, that scale would underflow to 0 in the
    reference, while the device's online log-sum-exp keeps a term down to e^-700: nothing to compare on.  No (distinct row,
    WD-stage star, grid) of the scripts is like that: a star with cooled nodes has one within 600 e-folds of its largest term."""
    from scipy.special import logsumexp
    ref = rcn.reference(setting, 1, 2)
    worst = 0.0
    for n_nodes in rcn.WD_NODES + (8, 16, 24):
        for nr in ref.wd_nodes(n_nodes, ref.distinct):
            for t, m, k, cooled, der in nr or ():
                if len(t) and cooled.any():
                    worst = max(worst, float(logsumexp(t) - t[cooled].max()))
    print(f"largest distance of a star's best cooled node below its log-sum: {worst:.3g} e-folds")
    assert worst < 600.0


@pytest.mark.parametrize("setting", list(rcn.SETTINGS))
def test_no_wd_stage_star_weighs_a_node_whose_precursor_age_is_ambiguous(setting):
    """The ladder pack's column of AGB-tip masses does not descend with age, which the WD branch's inversion for the precursor's
    age takes for granted: for a mass the column passes more than once the oracle's bisection and the device's 8-ary search may
    stop at different crossings, and neither is wrong (ragged_chain.tip_inversion_ambiguous).  No WD-stage star of the rung
    catalogue puts more than 1e-12 of its weight on such a node, at any distinct row of the scripts, on the 8 K steps of the
    chain_reduce calls or on the b9_wd_* calls' grids."""
    from scipy.special import logsumexp
    ref = rcn.reference(setting, 1, 2)
    prob = ref.prob
    worst, met = 0.0, 0
    for n_nodes in rcn.WD_NODES + (8, 16, 24):
        for par, nr in zip(ref.distinct, ref.wd_nodes(n_nodes, ref.distinct)):
            for t, m, k, cooled, der in nr or ():
                if not len(t):
                    continue
                amb = np.zeros(len(t), dtype=bool)
                for pop in np.unique(k):
                    amb[k == pop] = rcn.tip_inversion_ambiguous(prob["pack_d"], par, int(pop), m[k == pop])
                met += int(amb.sum())
                if amb.any():
                    worst = max(worst, float(np.exp(t - logsumexp(t))[amb].sum()))
    print(f"{met} (row, star, node) in the ambiguous band; the largest weight a star puts there: {worst:.3g}")
    assert worst <= 1e-12
