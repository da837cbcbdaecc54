"""CPU tests of the wdSummary host side: the symbols, b9h_wd_table against the formulas and tests/wdmoments_ref.py, the
.wdSummary file, the numpy reference's own sanity, the comparator of tests/wdmoments_check.py rejecting every mutation of
the reference, the conditions of the GPU tests' parity fixtures, and the statistical check of tests/test_gpu_wdmoments.py run
on numpy draws from the reference weights."""
import numpy as np
import pytest

import wdmoments_check as wc
import wdmoments_ref as wr
from base_amd import abi, hostlib


@pytest.fixture(scope="module")
def host():
    from base_amd import host_build
    host_build.build_host()
    return hostlib.load()


def test_symbols_are_listed():
    assert "b9_wd_moments" in abi.ABI_SYMBOLS
    assert "b9h_wd_table" in hostlib.HOST_SYMBOLS and "b9h_write_wd_summary" in hostlib.HOST_SYMBOLS
    assert abi.WDM_N == wr.N == 16 and abi.WDM_CONTINUE == 1
    names = ("ROWS", "MEMBER", "POP1", "COOLED", "M1", "M1SQ", "WDMASS", "WDMASS_SQ", "PREC", "PREC_SQ", "LOGCOOL", "LOGCOOL_SQ",
             "LOGTEFF", "LOGTEFF_SQ", "LOGG", "LOGG_SQ")
    assert [getattr(abi, "WDM_" + n) for n in names] == list(range(16)) == [getattr(wr, n) for n in names]
    assert len(hostlib.WD_TABLE_COLUMNS) == 16


def example_acc():
    rng = np.random.default_rng(6)
    n = 12
    rows = rng.integers(1, 50, n).astype(float)
    member = rows * rng.uniform(0.01, 1.0, n)
    cooled = member * rng.uniform(0.2, 1.0, n)
    mean = np.stack([rng.uniform(1.5, 7.0, n), rng.uniform(0.5, 1.2, n), rng.uniform(7.5, 9.5, n), rng.uniform(6.0, 9.6, n),
                     rng.uniform(3.6, 5.0, n), rng.uniform(7.0, 9.0, n)], axis=1)
    sd = rng.uniform(1e-3, 0.3, (n, 6))
    acc = np.zeros((n, 16))
    acc[:, wr.ROWS], acc[:, wr.MEMBER], acc[:, wr.COOLED], acc[:, wr.POP1] = rows, member, cooled, member * rng.uniform(0, 1, n)
    acc[:, wr.M1], acc[:, wr.M1SQ] = member * mean[:, 0], member * (sd[:, 0] ** 2 + mean[:, 0] ** 2)
    for q in range(5):
        acc[:, wr.WDMASS + 2 * q] = cooled * mean[:, 1 + q]
        acc[:, wr.WDMASS + 2 * q + 1] = cooled * (sd[:, 1 + q] ** 2 + mean[:, 1 + q] ** 2)
    acc[3] = 0.0; acc[3, wr.ROWS] = 7.0                                  # counted rows, no membership weight
    acc[4] = 0.0                                                         # a star no row contributed to
    acc[5, wr.COOLED] = 0.0; acc[5, wr.WDMASS:] = 0.0                     # membership weight, no cooled weight
    m = 1.2345678901234567                                               # a one-node posterior: the variance comes out slightly negative
    acc[6, wr.M1], acc[6, wr.M1SQ] = acc[6, wr.MEMBER] * m, acc[6, wr.MEMBER] * m * m * (1 - 2 ** -50)
    return acc, mean, sd


def test_wd_table_matches_formulas(host):
    acc, mean, sd = example_acc()
    t = hostlib.wd_table(acc)
    assert t.shape == (12, 16)
    np.testing.assert_array_equal(t[:, 0], acc[:, wr.ROWS])
    np.testing.assert_allclose(t, wr.table(acc), rtol=1e-15, atol=0)
    ok = np.ones(len(acc), bool); ok[[3, 4, 5, 6]] = False
    np.testing.assert_allclose(t[ok, 1], acc[ok, wr.MEMBER] / acc[ok, wr.ROWS], rtol=1e-15)
    np.testing.assert_allclose(t[ok, 2], acc[ok, wr.COOLED] / acc[ok, wr.MEMBER], rtol=1e-15)
    np.testing.assert_allclose(t[ok, 15], acc[ok, wr.POP1] / acc[ok, wr.MEMBER], rtol=1e-15)
    np.testing.assert_allclose(t[ok, 3], mean[ok, 0], rtol=1e-14)
    np.testing.assert_allclose(t[ok, 4], sd[ok, 0], rtol=1e-4)
    for q in range(5):
        np.testing.assert_allclose(t[ok, 5 + 2 * q], mean[ok, 1 + q], rtol=1e-14)
        np.testing.assert_allclose(t[ok, 6 + 2 * q], sd[ok, 1 + q], rtol=1e-3, atol=1e-6)       # (raw second moments of values near 9)
    # zeros for empty denominators
    assert t[3, 0] == 7 and np.all(t[3, 1:] == 0) and np.all(t[4] == 0)
    assert t[5, 1] > 0 and t[5, 2] == 0 and t[5, 3] > 0 and np.all(t[5, 5:15] == 0) and t[5, 15] > 0
    assert acc[6, wr.M1SQ] / acc[6, wr.MEMBER] - (acc[6, wr.M1] / acc[6, wr.MEMBER]) ** 2 < 0     # the raw variance IS negative ...
    assert t[6, 4] == 0.0 and t[6, 3] == pytest.approx(1.2345678901234567, rel=1e-15)            # ... and clamps to 0


@pytest.mark.parametrize("n_pops", [1, 2])
def test_wd_summary_round_trip(host, tmp_path, n_pops):
    acc, _, _ = example_acc()
    ids = [f"w{7 * i % 12:03d}" for i in range(len(acc))]                   # not sorted: the file keeps the caller's order
    path = str(tmp_path / "x.wdSummary")
    hostlib.write_wd_summary(path, ids, acc, n_pops)
    lines = open(path).read().splitlines()
    want_cols = list(hostlib.WD_TABLE_COLUMNS[:15]) + (["pPop2"] if n_pops == 2 else [])
    assert lines[0].split() == ["id"] + want_cols and len(lines) == 1 + len(acc)
    assert all(len(ln.split()) == 1 + len(want_cols) for ln in lines[1:])
    got_ids, cols, tab = hostlib.read_wd_summary(path)
    assert got_ids == ids and cols == want_cols
    np.testing.assert_allclose(tab, hostlib.wd_table(acc)[:, :len(want_cols)], rtol=0, atol=0.5e-6)
    assert np.array_equal(tab[:, 0], acc[:, 0])


# ---- the reference's own sanity -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """dsed, 5 filters, two populations of different tips (n_y = 3), 20 WD-stage stars, 4 rows, 48 nodes."""
    pack_d, cl, priors = wc.wd_problem("dsed", 5, 400, n_y=3, n_pops=2, keep=20)
    rows = wc.rows_for(cl, 4, 3, 2)
    rows[:, abi.P_LAMBDA] = [0.3, 0.5, 0.7, 0.2]
    rows[:, abi.P_Y2] = rows[:, abi.P_Y] + 0.04                           # two populations whose AGB tips differ
    return pack_d, cl, rows


def test_reference_agrees_with_itself(small):
    pack_d, cl, rows = small
    assert (np.asarray(cl["wd_type"]) == 1).any() and (np.asarray(cl["wd_type"]) == 0).any()
    one = wr.accumulate(pack_d, cl, rows, 2, 48)
    split = wr.accumulate(pack_d, cl, rows[1:], 2, 48, acc=wr.accumulate(pack_d, cl, rows[:1], 2, 48))
    assert np.array_equal(one, split)                                    # a split of the rows: the same bits
    assert np.all(one[:, wr.ROWS] == 4) and np.all(one[:, wr.COOLED] <= one[:, wr.MEMBER] * (1 + 1e-12))
    assert np.all(one[:, wr.POP1] <= one[:, wr.MEMBER] * (1 + 1e-12)) and np.any(one[:, wr.POP1] > 0)
    # a row outside the grid adds nothing
    out = rows[0].copy(); out[abi.P_LOGAGE] = pack_d["log_age"][-1] + 1.0
    assert np.all(wr.increments(pack_d, cl, out, 2, 48) == 0)
    # n_nodes = 1, one population: the increments are p (m, m^2, v, v^2) of the single node
    import moments_ref
    import numpy_ref
    import wd_check
    par = rows[0]
    x = wr.increments(pack_d, cl, par, 1, 1)
    t, m = numpy_ref.marg_terms_wd(pack_d, cl, par, 1, 0, n_nodes=1)
    v = np.array(wd_check.wd_chain(pack_d, par, m))[:, 0]
    assert v[1] < par[abi.P_LOGAGE]
    for c, i in enumerate(wr.wd_stars(cl)):
        p = moments_ref.membership(cl, i, t[i, 0])
        want = [1.0, p, 0.0, p, p * m[0], p * m[0] ** 2] + [p * y for q in range(5) for y in (v[q], v[q] ** 2)]
        np.testing.assert_allclose(x[c], want, rtol=1e-14, atol=0)


def test_comparator_rejects_every_mutation(small):
    """Each mutation on the fixture that can show it: the derived sums over all nodes need nodes that are not cooled (the seam
    fixture), the other four the two populations of different tips with DA and DB stars."""
    pack_d, cl, rows = small
    x, floor = wc.reference(pack_d, cl, rows, 2, 48)
    wc.assert_close(x, x, floor)
    wc.assert_close(x * (1 + 5e-10), x, floor)                           # inside the tolerance
    assert wc.rejects(wc.assert_close, x * (1 + 5e-9), x, floor)
    s_pack, s_cl, _, s_rows, s_nodes = wc.seam_fixture()
    sx, sfloor = wc.reference(s_pack, s_cl, s_rows, 1, s_nodes)
    for mutation in wr.MUTATIONS:
        kw = {mutation: 1 if mutation == "second_moment_power" else True}
        if mutation == "derived_over_all_nodes":
            bad, want, fl = np.stack([wr.increments(s_pack, s_cl, par, 1, s_nodes, **kw) for par in s_rows]), sx, sfloor
        else:
            bad, want, fl = np.stack([wr.increments(pack_d, cl, par, 2, 48, **kw) for par in rows]), x, floor
        assert wc.rejects(wc.assert_close, bad, want, fl), mutation
        assert wc.rejects(wc.assert_accumulated, bad.sum(axis=0), want, fl), mutation


def test_seam_fixture_has_cooled_weight_strictly_between_zero_and_member():
    pack_d, cl, _, rows, n_nodes = wc.seam_fixture()
    x, floor, amp = wr.increments(pack_d, cl, rows[0], 1, n_nodes, want_extra=True)
    share = x[:, wr.COOLED] / x[:, wr.MEMBER]
    print("cooled share of the membership weight:", share, "largest A", amp.max())
    assert np.all(x[:, wr.ROWS] == 1) and np.all(x[:, wr.MEMBER] > 1e-6) and amp.max() <= wc.A_MAX
    assert np.sum((share > 0.01) & (share < 0.99)) >= 3


# ---- the parity fixtures' conditions ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,largest", [("parsec", 56), ("dsed", 26), ("girardi", 7)])
def test_parity_fixture_conditions(key, largest):
    """Every (row, star) has at least one finite term and an amplification A <= 1e5: the GPU test leaves no pair out."""
    pack_d, cl, priors, rows, n_pops, n_nodes, x, floor, amp = wc.parity_fixture(key)
    assert x.shape == (6, 150, 16)
    print(f"{key}: largest A {amp.max():.3g}; pairs without a finite term {(amp < 0).sum()}; "
          f"COOLED == MEMBER bit for bit in {np.mean(x[..., wr.COOLED] == x[..., wr.MEMBER]):.1%} (to 1e-12 in all, asserted below)")
    assert np.all(x[..., wr.ROWS] == 1) and np.all(amp >= 0)
    assert amp.max() <= wc.A_MAX and amp.max() <= 2 * largest
    np.testing.assert_allclose(x[..., wr.COOLED], x[..., wr.MEMBER], rtol=1e-12, atol=0)


# ---- the statistical check of the GPU test, on numpy draws --------------------------------------------------------------------
def test_statistical_check_passes_on_numpy_draws_and_rejects_the_second_moment_mutant():
    import moments_ref
    tg = wc
    pack_d, cl, priors, rows = tg.stat_problem()
    nodes = wr.star_nodes(pack_d, cl, rows[0], 1, tg.STAT_NODES)[0]
    t, m, k, cooled, der = nodes
    w = np.exp(t - np.logaddexp.reduce(t))
    idx = np.random.default_rng(tg.STAT_SEED).choice(len(w), size=len(rows), p=w / w.sum())
    draws = dict(zams=m[idx], wd_mass=der[idx, 0], log_cool_age=der[idx, 2], log_teff=np.where(cooled[idx], der[idx, 3], 0.0))
    z = tg.stat_z(pack_d, cl, rows, draws, wr.table(wr.accumulate(pack_d, cl, rows[:1], 1, tg.STAT_NODES)))
    print("numpy draws, |z|:", np.abs(z))
    assert len(z) == 3 and np.all(np.abs(z) <= moments_ref.Z_MAX)
    z_mut = tg.stat_z(pack_d, cl, rows, draws, wr.table(wr.accumulate(pack_d, cl, rows[:1], 1, tg.STAT_NODES, second_moment_power=1)))
    assert not np.all(np.abs(z_mut) <= moments_ref.Z_MAX)
