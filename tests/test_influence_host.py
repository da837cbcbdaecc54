"""CPU tests of the starInfluence host side and of the checkers themselves: the header and the bindings; the recurrence of
tests/influence_ref.py against the same sums formed directly in long double; closed forms (q = 1, a one-star group);
b9h_influence_table / b9h_group_influence_table against the numpy restatements on synthetic v matrices pushed through the
reference's reducers; the comparators of tests/influence_check.py must accept the reference and reject nine mutated references;
starInfluence's flags, quantities and groups; the new kernels carry no scratch."""
import importlib.util
import math
import os
import re
import subprocess

import numpy as np
import pytest

import influence_check as ic
import influence_ref as ir
import pointwise_ref as pr
from base_amd import abi, hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host():
    from base_amd import host_build
    host_build.build_host()
    return hostlib.load()


@pytest.fixture(scope="module", autouse=True)
def the_call_exists():
    """Everything here checks b9_star_influence's statement or its host side: none of it stands without the call."""
    assert "b9_star_influence" in abi.ABI_SYMBOLS and "b9h_influence_table" in hostlib.HOST_SYMBOLS


def rejects(check, *args, **kw):
    try:
        check(*args, **kw)
    except AssertionError:
        return True
    return False


def tail_len_for(S):
    return min(256, min(S // 5, math.ceil(3 * math.sqrt(S))) + 1)


@pytest.fixture(scope="module")
def synthetic():
    """65 rows (one outside the grid) x 24 stars: log-likelihoods of a star's size whose spread grows with the star (so that the
    running maximum jumps often for the later ones), a star with v = -inf in one row, three quantities of which the first is
    correlated with the first stars' v; two groups and two stars in none."""
    rng = np.random.default_rng(11)
    n_rows, n = 65, 24
    q = rng.standard_normal((n_rows, 3))
    V = -30.0 + rng.standard_normal((n_rows, n)) * np.linspace(0.2, 4.0, n) + 0.8 * q[:, :1] * (np.arange(n) < 8)
    inside = np.ones(n_rows, bool); inside[7] = False
    V[7] = np.nan
    V[3, 4] = -np.inf
    group = (np.arange(n) % 2).astype(np.int32); group[[5, 6]] = -1
    return V, inside, q, group


# ---- the header and the bindings ----------------------------------------------------------------------------------------------
def test_header_library_and_binding_have_the_call():
    header = open(os.path.join(ROOT, "include", "base9_hip.h")).read()
    assert re.search(r"^int b9_star_influence\(", header, re.M) and "#define B9_ABI_VERSION 6" in header
    for name, value in (("ROWS", 0), ("NINF", 1), ("RMAX", 2), ("SNEG", 3), ("SNEG2", 4), ("MEANV", 5), ("HEAD", 6), ("MAX_Q", 12), ("MAX_GROUPS", 8), ("CONTINUE", 1)):
        assert re.search(r"^#define B9_INF_%s %d$" % (name, value), header, re.M), name
        assert getattr(abi, "INF_" + name) == value
    assert re.search(r"^#define B9_INF_WQ\(j\)\s+\(6 \+ 4 \* \(j\)\)", header, re.M) and re.search(r"^#define B9_INF_N\(Q\)\s+\(6 \+ 4 \* \(Q\)\)", header, re.M)
    assert abi.INF_WQ(2) == ir.WQ(2) == 14 and abi.INF_N(12) == ir.N(12) == 54
    lib = abi.load_hip_library()
    assert len(lib.b9_star_influence.argtypes) == 12
    out = subprocess.run(["nm", "-D", "--defined-only", abi.HIP_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "b9_star_influence" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


# ---- the reference against itself -----------------------------------------------------------------------------------------------
def test_recurrence_agrees_with_the_long_double_sums(synthetic):
    V, inside, q, _ = synthetic
    acc, (want, mag) = ir.accumulate(V, inside, q), ir.direct(V, inside, q)
    assert (acc[:, ir.SNEG] > 1.5).sum() >= 20 and acc[4, ir.NINF] == 1 and np.all(acc[:, ir.ROWS] == 64)
    ic.assert_acc(acc, want, V, inside, q)
    # ... far inside the bounds: the recurrence rounds, it does not drift
    live = slice(None)
    np.testing.assert_allclose(acc[live, ir.SNEG], want[live, ir.SNEG], rtol=1e-13)
    np.testing.assert_allclose(acc[:, ir.WQ(0) + 3], want[:, ir.WQ(0) + 3], rtol=1e-10, atol=1e-12)
    # any split of the rows carries the state whole
    part = ir.accumulate(V[:20], inside[:20], q[:20])
    assert np.array_equal(ir.accumulate(V[20:], inside[20:], q[20:], part), acc)


def test_unit_quantity_is_the_weights_own_sum(synthetic):
    V, inside, _, _ = synthetic
    acc = ir.accumulate(V, inside, np.ones((len(V), 2)))
    for j in range(2):
        assert np.array_equal(acc[:, ir.WQ(j)], acc[:, ir.SNEG]) and np.array_equal(acc[:, ir.WQ(j) + 1], acc[:, ir.SNEG])
        assert np.all(acc[:, ir.WQ(j) + 2] == 1.0) and np.all(acc[:, ir.WQ(j) + 3] == 0.0)


def test_a_one_star_group_is_that_star(synthetic, host):
    V, inside, q, _ = synthetic
    acc = ir.accumulate(V, inside, q)
    Vi, qi = V[inside], q[inside]
    for i in (0, 9, 23):
        group = np.full(V.shape[1], -1, np.int32); group[i] = 0
        L = ir.group_sums(Vi, np.ones(len(Vi), bool), group, 1)
        assert np.array_equal(L[:, 0], Vi[:, i])
        for tab in (ir.group_table(L, qi, group), hostlib.group_influence_table(L, qi, group)):
            assert tab[0, 0] == 1 and tab[0, 1] == 64 and tab[0, 2] == 0
            for j in range(3):
                m = acc[i, ir.WQ(j)] / acc[i, ir.SNEG]
                assert abs(tab[0, ir.GROUP_HEAD + 3 * j] + qi[:, j].mean() - m) <= 1e-12
            assert abs(tab[0, 3] - acc[i, ir.SNEG] ** 2 / acc[i, ir.SNEG2]) <= 1e-10 * tab[0, 3]


# ---- the host tables ------------------------------------------------------------------------------------------------------------
def test_tables_against_numpy(synthetic, host):
    V, inside, q, group = synthetic
    T = tail_len_for(64)
    assert T == 13
    acc, tail = ir.accumulate(V, inside, q), pr.top_tail(V, inside, T)
    want = ir.table(V, inside, q, n_keep=T)
    got = hostlib.influence_table(acc, tail)
    assert got.shape == (24, 13) and np.isfinite(want[:, 3]).sum() >= 20 and (np.abs(want[:, ir.STAR_HEAD]) > 1e-3).sum() >= 20
    ic.assert_table(got, want, V, inside, q)
    assert got[4, 1] == 1 and got[4, 2] == 0 and np.all(np.isnan(got[4, 3:]))                       # nInf > 0
    no_tail = hostlib.influence_table(acc)
    assert np.all(np.isnan(no_tail[:, 3])) and np.array_equal(np.delete(no_tail, 3, axis=1), np.delete(got, 3, axis=1), equal_nan=True)
    assert np.all(hostlib.influence_table(np.zeros((3, ir.N(2)))) == 0)                                 # rows = 0
    # lin is the first-order form of shift: the two agree where the weights are nearly even
    Vs = -30.0 + 0.05 * (V[inside][:, :4] + 30.0) / np.linspace(0.2, 4.0, 24)[:4] + 0.05 * q[inside][:, :1]
    small = hostlib.influence_table(ir.accumulate(Vs, None, q[inside]))
    assert np.all(small[:, 2] > 60) and np.all(np.abs(small[:, ir.STAR_HEAD + 1]) > 0.02)
    assert np.all(np.abs(small[:, ir.STAR_HEAD] - small[:, ir.STAR_HEAD + 1]) <= 0.1 * np.abs(small[:, ir.STAR_HEAD + 1]))

    L = ir.group_sums(V, inside, group, 2)[inside]
    wantg, gotg = ir.group_table(L, q[inside], group), hostlib.group_influence_table(L, q[inside], group)
    assert list(wantg[:, 0]) == [11, 11] and wantg[1, 2] == 0 and np.isfinite(wantg[1, 4])
    assert wantg[0, 2] == 1 and wantg[0, 3] == 0 and np.all(np.isnan(wantg[0, 4:]))                 # star 4's -inf row is in group 0
    ic.assert_group_table(gotg, wantg)
    assert wantg[1, ir.GROUP_HEAD] != wantg[1, ir.GROUP_HEAD + 1]                                     # the smoothing moved the shift
    L0 = ir.group_sums(np.delete(V, 4, axis=1), inside, np.delete(group, 4), 2)[inside]
    ic.assert_group_table(hostlib.group_influence_table(L0, q[inside], np.delete(group, 4)), ir.group_table(L0, q[inside], np.delete(group, 4)))
    # too few rows for a fit: shift = shiftRaw, paretoK NaN
    few = hostlib.group_influence_table(L0[:12], q[inside][:12], np.delete(group, 4))
    assert np.all(np.isnan(few[:, 4])) and np.array_equal(few[:, ir.GROUP_HEAD], few[:, ir.GROUP_HEAD + 1])
    ic.assert_group_table(few, ir.group_table(L0[:12], q[inside][:12], np.delete(group, 4)))


# ---- the comparators reject the mutants -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", ir.MUTANTS)
def test_rejects_a_faulty_recurrence(synthetic, mutant):
    """WQ2 not rescaled at a jump; f for f f in SNEG2; the old mean in CVQ; -inf rows counted in k; k for k + 1."""
    V, inside, q, _ = synthetic
    want = ir.accumulate(V, inside, q)
    ic.assert_acc(want, want, V, inside, q)
    bad = ir.accumulate(V, inside, q, mutant=mutant)
    assert rejects(ic.assert_acc, bad, want, V, inside, q)
    if mutant == "inf_counts_in_k":                       # only the star with a -inf row shows it
        assert np.array_equal(np.delete(bad, 4, axis=0), np.delete(want, 4, axis=0))


def test_rejects_group_ids_ignored(synthetic):
    V, inside, _, group = synthetic
    want = ir.group_sums(V, inside, group, 2)
    ic.assert_groups(want, want, V, inside, group)
    assert rejects(ic.assert_groups, ir.group_sums(V, inside, group, 2, ignore_ids=True), want, V, inside, group)


@pytest.mark.parametrize("mutation", [dict(sign_shift=-1.0), dict(sign_lin=1.0), dict(ess_plain=True)], ids=["sign_of_shift", "sign_of_lin", "ess_as_SNEG_over_SNEG2"])
def test_rejects_a_faulty_table(synthetic, mutation):
    V, inside, q, group = synthetic
    want = ir.table(V, inside, q, n_keep=13)
    ic.assert_table(want, want, V, inside, q)
    assert rejects(ic.assert_table, ir.table(V, inside, q, n_keep=13, **mutation), want, V, inside, q)
    if "sign_lin" not in mutation:                        # (the group table has no lin)
        L = ir.group_sums(V, inside, group, 2)[inside]
        assert rejects(ic.assert_group_table, ir.group_table(L, q[inside], group, **mutation), ir.group_table(L, q[inside], group))


# ---- the program's settings, quantities and groups ----------------------------------------------------------------------------------
def test_flags_quantities_and_groups(host, tmp_path):
    assert hostlib.star_influence_settings([]) == dict(margIsoIncrem=4, nMassRatios=4, nPops=1, quantity=[], groupFile="", noGroups=0)
    d = hostlib.star_influence_settings(["--quantity", "logAge", "--quantity", "logPost", "--nPops", "2", "--noGroups", "--margIsoIncrem=2"])
    assert d == dict(margIsoIncrem=2, nMassRatios=4, nPops=2, quantity=["logAge", "logPost"], groupFile="", noGroups=1)
    y = tmp_path / "s.yaml"
    y.write_text("starInfluence:\n  quantity: logAge Av\n  groupFile: groups.txt\n")
    assert hostlib.star_influence_settings(["--config", str(y)])["quantity"] == ["logAge", "Av"]
    assert hostlib.star_influence_settings(["--config", str(y)])["groupFile"] == "groups.txt"
    with pytest.raises(hostlib.HostError, match="at most 12"):
        hostlib.star_influence_settings(sum((["--quantity", "logAge"] for _ in range(13)), []))
    with pytest.raises(hostlib.HostError, match="not both"):
        hostlib.star_influence_settings(["--noGroups", "--groupFile", "g"])

    rng = np.random.default_rng(2)
    rows = np.tile(np.arange(abi.B9_NPARAM, dtype=np.float64), (50, 1))
    rows[:, abi.P_LOGAGE] += 0.01 * rng.standard_normal(50)
    rows[:, abi.P_MOD] += 0.1 * rng.standard_normal(50)
    lp = rng.standard_normal(50)
    names, q, mean, sd = hostlib.influence_quantities([], rows, lp)                                 # default: the parameters that vary, in B9_P_* order
    order = sorted([abi.P_LOGAGE, abi.P_MOD])
    want, wmean, wsd = ir.zscores(rows[:, order])
    assert len(names) == 2 and np.allclose(q, want, rtol=1e-13, atol=1e-13) and np.allclose(mean, wmean, rtol=1e-15) and np.allclose(sd, wsd, rtol=1e-14)
    names2, q2, _, _ = hostlib.influence_quantities(["--quantity", "logPost", "--quantity", names[0]], rows, lp)
    assert names2 == ["logPost", names[0]] and np.allclose(q2[:, 0], ir.zscores(lp[:, None])[0][:, 0], rtol=1e-13, atol=1e-13) and np.array_equal(q2[:, 1], q[:, 0])
    for bad, msg in ((["--quantity", "nonsense"], "neither"), (["--quantity", names[0]] * 13, "at most 12")):
        with pytest.raises(hostlib.HostError, match=msg):
            hostlib.influence_quantities(bad, rows, lp)
    with pytest.raises(hostlib.HostError, match="does not vary"):
        hostlib.influence_quantities(["--quantity", names[0]], np.tile(rows[:1], (50, 1)), lp)

    ids, stage = ["a", "b", "c", "d"], [abi.STAGE_MSRG, abi.STAGE_WD, abi.STAGE_MSRG, abi.STAGE_BD]
    gn, g = hostlib.influence_groups([], ids, stage)
    assert gn == ["ms", "wd"] and list(g) == [0, 1, 0, -1]
    assert hostlib.influence_groups(["--noGroups"], ids, stage)[0] == []
    gf = tmp_path / "groups.txt"
    gf.write_text("c turnoff\na giants\n# a comment\nd turnoff\n")
    gn, g = hostlib.influence_groups(["--groupFile", str(gf)], ids, stage)
    assert gn == ["turnoff", "giants"] and list(g) == [1, -1, 0, 0]
    gf.write_text("c turnoff\nzz giants\n")
    with pytest.raises(hostlib.HostError, match="unknown star id 'zz'"):
        hostlib.influence_groups(["--groupFile", str(gf)], ids, stage)
    gf.write_text("".join(f"a g{k}\n" for k in range(9)))
    with pytest.raises(hostlib.HostError, match="at most 8"):
        hostlib.influence_groups(["--groupFile", str(gf)], ids, stage)


def test_files_read_back_to_the_bits(host, synthetic, tmp_path):
    V, inside, q, group = synthetic
    tab = hostlib.influence_table(ir.accumulate(V, inside, q), pr.top_tail(V, inside, 13))
    ids, names = [f"s{i}" for i in range(24)], ["logAge", "Av", "logPost"]
    hostlib.write_star_influence(str(tmp_path / "x.starInfluence"), ids, names, tab)
    rid, cols, back = hostlib.read_star_influence(str(tmp_path / "x.starInfluence"))
    assert rid == ids and cols[:4] == list(hostlib.INFLUENCE_HEAD) and cols[4:7] == ["shift_logAge", "lin_logAge", "looSd_logAge"] and len(cols) == 13
    assert np.array_equal(back, tab, equal_nan=True)
    gt = hostlib.group_influence_table(ir.group_sums(V, inside, group, 2)[inside], q[inside], group)
    hostlib.write_group_influence(str(tmp_path / "x.groupInfluence"), ["ms", "wd"], names, gt)
    gid, cols, back = hostlib.read_group_influence(str(tmp_path / "x.groupInfluence"))
    assert gid == ["ms", "wd"] and cols[:5] == list(hostlib.GROUP_INFLUENCE_HEAD) and cols[5:8] == ["shiftRaw_logAge", "shift_logAge", "looSd_logAge"]
    assert np.array_equal(back, gt, equal_nan=True)


# ---- the kernels --------------------------------------------------------------------------------------------------------------------
def test_no_influence_kernel_has_a_private_segment():
    """Every k_infl_* instance of the shipped header, compiled to gfx950 assembly: .amdhsa_private_segment_fixed_size 0."""
    spec = importlib.util.spec_from_file_location("check_async_sloads", os.path.join(ROOT, "tools", "check_async_sloads.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    scratch, cur = {}, None
    for line in open(chk.device_asm()):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            cur = m.group(1)
            continue
        m = re.match(r"\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", line)
        if m and cur:
            scratch[cur] = int(m.group(1))
    # Itanium names: k_infl_accumulate<QT> = _Z17k_infl_accumulateILi<QT>EE..., k_infl_groups<NG> = _Z13k_infl_groupsILi<NG>EE...
    for stem, sizes in (("_Z17k_infl_accumulateILi%dEE", (1, 2, 4)), ("_Z13k_infl_groupsILi%dEE", (1, 2, 4, 8))):
        for k in sizes:
            hit = [name for name in scratch if name.startswith(stem % k)]
            assert len(hit) == 1, (stem % k, hit)
            assert scratch[hit[0]] == 0, (hit[0], scratch[hit[0]])
