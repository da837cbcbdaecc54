"""CPU tests of the modelScore host side and of the checkers themselves: closed forms of the reference (tests/pointwise_ref.py);
b9h_pointwise_table / b9h_score_totals / b9h_score_compare against the numpy restatements on synthetic v matrices pushed through
the reference's accumulate; recovery of a known Pareto tail index; the comparators of tests/pointwise_check.py must accept the
reference and reject six mutated references, each on a case where the reference itself shows that the mutation matters;
modelScore's flags and YAML keys; --compareTo on hand-written .pointwise files."""
import math
import os
import subprocess

import numpy as np
import pytest

import pointwise_check as pc
import pointwise_ref as pr
from base_amd import abi, hostlib, synth
from conftest import build_problem


@pytest.fixture(scope="module")
def host():
    from base_amd import host_build
    host_build.build_host()
    return hostlib.load()


@pytest.fixture(scope="module", autouse=True)
def the_call_exists():
    """Everything here checks b9_pointwise's statement or its host side: none of it stands without the call."""
    assert "b9_pointwise" in abi.ABI_SYMBOLS and "b9h_pointwise_table" in hostlib.HOST_SYMBOLS


def rejects(check, *args, **kw):
    try:
        check(*args, **kw)
    except AssertionError:
        return True
    return False


def tail_len_for(S):
    return min(256, min(S // 5, math.ceil(3 * math.sqrt(S))) + 1)


def through_acc(V, T, inside=None):
    """(acc, tail) of the reference's reducers: what the call would hand the host library."""
    inside = np.ones(len(V), bool) if inside is None else inside
    return pr.accumulate(V, inside), pr.top_tail(V, inside, T)


# ---- closed forms -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [20, 100])
def test_identical_rows(host, S):
    """S identical rows: lppd = elpdIs = elpdLoo = v, pWaic = 0, no fit (S = 20: the tail is too short; S = 100: it has no spread)."""
    c = -37.25
    V = np.full((S, 3), c)
    V[:, 1] = 2.5
    V[:, 2] = 0.0
    want, _ = pr.table(V)
    for tab in (want, hostlib.pointwise_table(*through_acc(V, tail_len_for(S)))):
        for i, x in enumerate((c, 2.5, 0.0)):
            np.testing.assert_allclose(tab[i, [pr.T_LPPD, pr.T_ELPD_WAIC, pr.T_ELPD_IS, pr.T_ELPD_LOO]], x, rtol=0, atol=1e-13)
            assert tab[i, pr.T_ROWS] == S and tab[i, pr.T_NINF] == 0 and abs(tab[i, pr.T_PWAIC]) < 1e-25 and np.isnan(tab[i, pr.T_K])


def test_two_values_by_hand(host):
    a, b = -1.0, -3.0
    V = np.array([[a], [b]])
    acc = pr.accumulate(V)
    e2 = math.exp(-2.0)
    np.testing.assert_allclose(acc[0], [2, 0, a, 1 + e2, -b, 1 + e2, -2.0, 2.0], rtol=1e-15)
    lppd = math.log((math.exp(a) + math.exp(b)) / 2)
    elpd_is = math.log(2) - math.log(math.exp(-a) + math.exp(-b))          # the harmonic mean of the two likelihoods
    want = [2, 0, lppd, 2.0, lppd - 2.0, elpd_is, np.nan, elpd_is, lppd - elpd_is]
    ref, _ = pr.table(V)
    np.testing.assert_allclose(ref[0], want, rtol=1e-14, equal_nan=True)
    np.testing.assert_allclose(hostlib.pointwise_table(acc, pr.top_tail(V, np.ones(2, bool), 1))[0], want, rtol=1e-14, equal_nan=True)
    # the other order: the same multiset, VMAX / RMAX reached by the jump instead
    acc2 = pr.accumulate(V[::-1])
    np.testing.assert_allclose(acc2[0], [2, 0, a, 1 + e2, -b, 1 + e2, -2.0, 2.0], rtol=1e-15)
    # a -inf row counts in ROWS and NINF and touches nothing else; it makes every leave-one-out score -inf
    acc3 = pr.accumulate(np.array([[a], [-np.inf], [b]]))
    assert acc3[0, 0] == 3 and acc3[0, 1] == 1 and np.array_equal(acc3[0, 2:], acc[0, 2:])
    t3 = hostlib.pointwise_table(acc3, None)[0]
    assert t3[pr.T_ELPD_WAIC] == t3[pr.T_ELPD_IS] == t3[pr.T_ELPD_LOO] == -np.inf and t3[pr.T_K] == np.inf
    np.testing.assert_allclose(t3[pr.T_LPPD], math.log((math.exp(a) + math.exp(b)) / 3), rtol=1e-14)
    np.testing.assert_array_equal(t3, pr.table(np.array([[a], [-np.inf], [b]]))[0][0])


# ---- the host tables against the numpy restatements --------------------------------------------------------------------------
def synthetic(S=200, n=30, seed=5):
    """v matrices with every kind of star: Gaussian spread of several widths, exponential (Pareto-weight) tails of index 0.2 ..
    0.9, ties, a star with a -inf row, a star no row counted (through `inside` it cannot be made: it is zeroed in acc)."""
    rng = np.random.default_rng(seed)
    V = rng.normal(0, 1, (S, n)) * rng.uniform(0.05, 1.5, n) + rng.uniform(-60, 5, n)
    for i, k in zip(range(10, 18), np.linspace(0.2, 0.9, 8)):
        V[:, i] = -20.0 - k * rng.exponential(1.0, S)
    V[:, 18] = np.round(V[:, 18], 1)                      # ties
    V[7, 19] = -np.inf
    return V


def test_tables_against_numpy(host):
    V = synthetic()
    S, n = V.shape
    T = tail_len_for(S)
    assert T == 41
    acc, tail = through_acc(V, T)
    acc[20], tail[20] = 0.0, -np.inf                       # never counted
    got = hostlib.pointwise_table(acc, tail)
    want, ratio = pr.table(V)
    want[20] = 0.0
    fitted = np.isfinite(want[:, pr.T_K]) & (want[:, pr.T_ROWS] > 0)
    print(f"{fitted.sum()} fitted stars, paretoK {np.nanmin(want[fitted, pr.T_K]):.3f} .. {np.nanmax(want[fitted, pr.T_K]):.3f}, "
          f"largest SNEG / den {np.nanmax(ratio):.3g}")
    assert fitted.sum() >= 25 and (want[fitted, pr.T_K] > 0.7).sum() >= 1 and (want[fitted, pr.T_K] < 0.3).sum() >= 5
    assert np.nanmax(ratio) <= 1e3                         # the subtraction in `den` loses 2^-52 SNEG / den: stated before the comparison
    assert np.all(got[20] == 0) and got[19, pr.T_NINF] == 1 and got[19, pr.T_ELPD_LOO] == -np.inf and got[19, pr.T_K] == np.inf
    pc.assert_table(got, want, tol=1e-12, loo_tol=1e-9)
    # the smoothing matters: elpdLoo is not elpdIs on most fitted stars
    assert (np.abs(want[fitted, pr.T_ELPD_LOO] - want[fitted, pr.T_ELPD_IS]) > 1e-4).sum() >= 20
    # a tail kept longer than needed changes nothing; without a tail no fit is made
    longer = hostlib.pointwise_table(acc, np.where(np.arange(n)[:, None] == 20, -np.inf, pr.top_tail(V, np.ones(S, bool), 64)))
    assert np.array_equal(longer, got, equal_nan=True)
    none = hostlib.pointwise_table(acc, None)
    assert np.all(np.isnan(none[fitted, pr.T_K])) and np.array_equal(none[fitted, pr.T_ELPD_LOO], none[fitted, pr.T_ELPD_IS])

    tot, want_tot = hostlib.score_totals(got), pr.totals(want)
    assert list(tot) == list(hostlib.SCORE_TOTALS)
    g = np.array([tot[k] for k in hostlib.SCORE_TOTALS])
    assert g[0] == n - 1 and g[9] == 1 and g[10] == want_tot[10] >= 1 and g[5] == -np.inf
    ok = np.isfinite(want_tot)
    np.testing.assert_allclose(g[ok], want_tot[ok], rtol=1e-12)
    assert np.array_equal(g[~ok], want_tot[~ok], equal_nan=True)
    # the finite stars alone: every total is a number
    keep = np.arange(n) != 19
    tot = hostlib.score_totals(got[keep])
    np.testing.assert_allclose([tot[k] for k in hostlib.SCORE_TOTALS], pr.totals(want[keep]), rtol=1e-9)
    np.testing.assert_allclose([tot[k] for k in hostlib.SCORE_TOTALS][:5], pr.totals(want[keep])[:5], rtol=1e-12)


def test_compare_against_numpy(host):
    Va, Vb = synthetic(seed=5), synthetic(seed=5)
    Vb[:, :10] += np.random.default_rng(2).normal(0.1, 0.05, 10)          # model B predicts the first ten stars a little better
    keep = np.arange(Va.shape[1]) != 19
    Va, Vb = Va[:, keep], Vb[:, keep]
    ta, tb = (hostlib.pointwise_table(*through_acc(V, 41)) for V in (Va, Vb))
    ids = [f"s{i}" for i in range(Va.shape[1])]
    got = hostlib.score_compare(ta, ids, tb, ids)
    assert list(got) == list(hostlib.SCORE_COMPARE)
    (ref_a, ratio_a), (ref_b, ratio_b) = pr.table(Va), pr.table(Vb)
    print(f"largest SNEG / den: {np.nanmax(ratio_a):.3g} (A), {np.nanmax(ratio_b):.3g} (B)")
    assert np.nanmax(ratio_a) <= 1e3 and np.nanmax(ratio_b) <= 1e3      # stated before any elpdLoo is compared at 1e-9
    want = pr.compare(ref_a, ref_b)
    assert got["nStars"] == want[0] == 29 and got["nDropped"] == want[5] == 0
    np.testing.assert_allclose([got["dElpdWaic"], got["dElpdWaicSe"]], want[3:5], rtol=1e-12, atol=0)
    np.testing.assert_allclose([got["dElpdLoo"], got["dElpdLooSe"]], want[1:3], rtol=1e-9, atol=0)
    # a star only one fit scored leaves the differences and is counted
    tz = tb.copy(); tz[3] = 0.0
    rz = ref_b.copy(); rz[3] = 0.0
    got_z, want_z = hostlib.score_compare(ta, ids, tz, ids), pr.compare(ref_a, rz)
    assert got_z["nStars"] == want_z[0] == 28 and got_z["nDropped"] == want_z[5] == 1
    np.testing.assert_allclose([got_z["dElpdWaic"], got_z["dElpdWaicSe"]], want_z[3:5], rtol=1e-12, atol=0)
    assert got["dElpdLoo"] < -3 * got["dElpdLooSe"] < 0 and got["dElpdWaic"] < 0
    other = list(ids); other[3], other[4] = other[4], other[3]
    for bad in (other, ids[:-1], ids[:5] + ["x"] + ids[6:]):
        with pytest.raises(hostlib.HostError, match="differ"):
            hostlib.score_compare(ta, ids, tb[:len(bad)], bad)


# ---- recovery of a known tail index -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0.2, 0.7])
def test_pareto_tail_index_is_recovered(host, k):
    """r_s = k E_s with E standard exponential: e^r is Pareto with shape k.  S = 4000 rows give M = 190 tail values, so the
    estimator's standard deviation is about (1 + k) / sqrt(M) ~ 0.1: |k_hat - k| <= 0.35, on the numpy statement first."""
    S = 4000
    r = k * np.random.default_rng(20240611).exponential(1.0, S)
    V = -r[:, None]
    assert pr.tail_length(S, S) == 190
    k_ref, _, _ = pr.psis(V[:, 0])
    print(f"k = {k}: the reference estimates {k_ref:.4f}")
    assert abs(k_ref - k) <= 0.35
    got = hostlib.pointwise_table(*through_acc(V, 191))
    assert abs(got[0, pr.T_K] - k) <= 0.35
    np.testing.assert_allclose(got[0, pr.T_K], k_ref, rtol=1e-9)


# ---- the comparators reject mutated references ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case1():
    """Case 1 of tests/test_gpu_moments.py (dsed, 5 filters, two populations, 130 stars, 2 x 2 grid), lambda = 0.3, and its V."""
    pack_d, cl, pack, stars, priors, _ = build_problem("dsed", 5, n_stars=130, wd_frac=0.1, n_y=3, n_pops=2, seed=12)
    rows = synth.walker_params(cl["truth"], 3, seed=3, scale=0.3)
    rows[:, abi.P_LAMBDA] = 0.3
    return pack_d, cl, rows, pr.v_matrix(pack_d, cl, rows, 2, 2, 2)


def test_comparators_accept_the_reference(case1):
    pack_d, cl, rows, (V, inside, live) = case1
    n = V.shape[1]
    acc, tail, rws = pr.accumulate(V, inside), pr.top_tail(V, inside, 2), pr.row_sums(V, inside)
    for f in (1.0, 1 + 1e-10):                             # ... and a copy perturbed at a tenth of the tolerance
        pc.assert_values(V * f, V)
        a = acc.copy(); a[:, [pr.VMAX, pr.RMAX, pr.MEAN]] *= f
        pc.assert_acc(a, acc)
        pc.assert_tail(tail * f, tail)
        pc.assert_rows(rws * f, rws, n)
    assert rejects(pc.assert_values, V * (1 + 1e-8), V) and rejects(pc.assert_rows, rws * (1 + 1e-8), rws, n)
    m2, wd = pc.non_vacuity(acc, cl, live)
    print(f"{m2} of {n} stars with M2 > 0, {wd} live WD-stage stars")
    assert m2 >= (9 * n) // 10 and wd >= 1


def test_rejects_field_term_dropped(case1):
    pack_d, cl, rows, (V, inside, live) = case1
    got, _, _ = pr.v_matrix(pack_d, cl, rows, 2, 2, 2, drop_field=True)
    d = pc.largest(got, V)
    print(f"field term dropped: largest difference {d:.3g}")
    assert d > 1e-3
    assert rejects(pc.assert_values, got, V) and rejects(pc.assert_acc, pr.accumulate(got, inside), pr.accumulate(V, inside))
    assert rejects(pc.assert_rows, pr.row_sums(got, inside), pr.row_sums(V, inside), V.shape[1])


def test_rejects_population_weight_dropped(case1):
    pack_d, cl, rows, (V, inside, live) = case1
    got, _, _ = pr.v_matrix(pack_d, cl, rows, 2, 2, 2, drop_pop_weight=True)
    d = pc.largest(got, V)
    print(f"log lambda_k dropped: largest difference {d:.3g}")
    assert d > 1e-3
    assert rejects(pc.assert_values, got, V) and rejects(pc.assert_tail, pr.top_tail(got, inside, 2), pr.top_tail(V, inside, 2))


def test_rejects_rows_without_a_live_node_skipped():
    """A parametrised IFMR that gives M_wd <= 0 at every node: the row's WD-stage stars have no node, and still count."""
    pack_d, cl, pack, stars, priors, _ = build_problem("parsec", 4, n_stars=70, wd_frac=0.1, seed=12, ifmr_id=abi.IFMR_LINEAR)
    rows = synth.walker_params(cl["truth"], 3, seed=3, scale=0.3)
    rows[1, abi.P_IFMR_INTERCEPT], rows[1, abi.P_IFMR_SLOPE] = -10.0, 0.0
    V, inside, live = pr.v_matrix(pack_d, cl, rows, 1, 2, 2)
    wd = np.asarray(cl["stage"]) == abi.STAGE_WD
    assert wd.sum() >= 3 and inside.all() and not live[1, wd].any() and live[0, wd].any() and live[:, ~wd].all()
    for i in np.flatnonzero(wd):
        assert V[1, i] == pr.field_term(cl, i)            # the field term, exactly
    want = pr.accumulate(V, inside)
    got = pr.accumulate(V, inside, skip=~live)
    assert np.all(want[:, pr.ROWS] == 3) and np.all(got[wd, pr.ROWS] == 2)
    pc.assert_acc(want, want)
    assert rejects(pc.assert_acc, got, want)


def test_rejects_m2_from_the_old_mean(case1):
    pack_d, cl, rows, (V, inside, live) = case1
    want, got = pr.accumulate(V, inside), pr.accumulate(V, inside, m2_from_old_mean=True)
    rel = np.abs(got[:, pr.M2] - want[:, pr.M2]) / np.maximum(want[:, pr.M2], 1e-300)
    print(f"M2 from (v - mean_old)^2: relative difference {rel[want[:, pr.M2] > 0].min():.3g} .. {rel.max():.3g}")
    assert (rel > 0.1).sum() >= 100
    assert np.array_equal(got[:, :pr.M2], want[:, :pr.M2])                # nothing else moves: M2's own bound must catch it
    assert rejects(pc.assert_acc, got, want)


def test_rejects_tail_ascending(case1):
    pack_d, cl, rows, (V, inside, live) = case1
    want, got = pr.top_tail(V, inside, 3), pr.top_tail(V, inside, 3, ascending=True)
    assert (want[:, 0] - want[:, 2] > 1e-6).sum() >= 100
    pc.assert_tail(want, want)
    assert rejects(pc.assert_tail, got, want)
    assert rejects(pc.assert_tail, np.sort(want, axis=1), want)


def test_rejects_shrinkage_left_out():
    V = synthetic()[:, :19]
    want, _ = pr.table(V)
    got, _ = pr.table(V, shrink=False)
    fitted = np.isfinite(want[:, pr.T_K])
    d = np.abs(got[fitted, pr.T_K] - want[fitted, pr.T_K])
    print(f"the prior on k left out: paretoK moves by {d.min():.3g} .. {d.max():.3g}")
    assert fitted.sum() >= 15 and d.min() > 1e-3
    pc.assert_table(want, want)
    assert rejects(pc.assert_table, got, want)


# ---- flags and YAML -----------------------------------------------------------------------------------------------------------
def test_flags_and_yaml_parse(host, tmp_path):
    assert hostlib.model_score_settings([]) == dict(margIsoIncrem=4, nMassRatios=4, nPops=1, perRow=0, compareTo="")
    d = hostlib.model_score_settings(["--perRow", "--nPops", "2", "--margIsoIncrem", "2", "--nMassRatios=3", "--compareTo", "other/run"])
    assert d == dict(margIsoIncrem=2, nMassRatios=3, nPops=2, perRow=1, compareTo="other/run")
    y = tmp_path / "ms.yaml"
    y.write_text("sampleMass:\n  margIsoIncrem: 6\n  nMassRatios: 5\nphotResiduals:\n  nPops: 2\nsimCluster:\n  nPops: 2\n"
                 "modelScore:\n  nMassRatios: 7\n")
    d = hostlib.model_score_settings(["--config", str(y)])                  # sampleMass's grid is the default; other programs' keys are not read
    assert d == dict(margIsoIncrem=6, nMassRatios=7, nPops=1, perRow=0, compareTo="")
    y.write_text("modelScore:\n  margIsoIncrem: 3\n  nMassRatios: 2\n  nPops: 2\n  perRow: 1\n")
    assert hostlib.model_score_settings(["--config", str(y)]) == dict(margIsoIncrem=3, nMassRatios=2, nPops=2, perRow=1, compareTo="")
    assert hostlib.model_score_settings(["--config", str(y), "--perRow=0", "--nPops=1"]) == dict(margIsoIncrem=3, nMassRatios=2, nPops=1, perRow=0, compareTo="")
    for bad in (["--nPops", "3"], ["--margIsoIncrem", "0"], ["--nMassRatios", "0"]):
        with pytest.raises(hostlib.HostError):
            hostlib.model_score_settings(bad)


# ---- --compareTo: no GPU ------------------------------------------------------------------------------------------------------
def _model_score(*args):
    from base_amd import host_build
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    return subprocess.run([os.path.join(host_build.BIN, "modelScore"), *args], capture_output=True, text=True, timeout=120, env=env)


def test_compare_to_on_hand_written_files(host, tmp_path):
    header = "id " + " ".join(hostlib.POINTWISE_COLUMNS) + "\n"
    # id rows nInf lppd pWaic elpdWaic elpdIs paretoK elpdLoo pLoo
    a = [("s1", 10, 0, -3.0, 0.5, -3.5, -3.4, 0.1, -3.25, 0.25), ("s2", 10, 0, -5.0, 1.0, -6.0, -5.5, "nan", -5.5, 0.5),
         ("s3", 10, 0, -1.0, 0.25, -1.25, -1.2, 0.3, -1.125, 0.125), ("s4", 0, 0, 0, 0, 0, 0, 0, 0, 0)]
    b = [("s1", 10, 0, -3.5, 0.5, -4.0, -3.9, 0.1, -4.0, 0.5), ("s2", 10, 0, -5.0, 0.5, -5.5, -5.2, 0.2, -5.25, 0.25),
         ("s3", 10, 0, -2.0, 0.5, -2.5, -2.4, 0.3, -2.625, 0.625), ("s4", 10, 0, -9.0, 0, -9.0, -9.0, 0.0, -9.0, 0)]
    for name, tab in (("a", a), ("b", b)):
        with open(tmp_path / f"{name}.pointwise", "w") as f:
            f.write(header + "".join(" ".join(str(x) for x in line) + "\n" for line in tab))
    base_a, base_b = str(tmp_path / "a"), str(tmp_path / "b")
    r = _model_score("--outputFileBase", base_a, "--compareTo", base_b)
    assert r.returncode == 0, r.stderr
    # by hand: s4 was never counted under A and stays out; LOO differences 0.75, -0.25, 1.5; WAIC 0.5, -0.5, 1.25
    d_loo, d_waic = np.array([0.75, -0.25, 1.5]), np.array([0.5, -0.5, 1.25])
    want = dict(nStars=3, dElpdLoo=d_loo.sum(), dElpdLooSe=math.sqrt(3 * d_loo.var(ddof=1)), dElpdWaic=d_waic.sum(),
                dElpdWaicSe=math.sqrt(3 * d_waic.var(ddof=1)), nDropped=1)
    got = hostlib.read_named_values(base_a + ".modelCompare")
    assert list(got) == list(hostlib.SCORE_COMPARE)
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-14), k
    assert "2.000000 +-" in r.stdout and "1.250000 +-" in r.stdout and "1 star(s) scored by one of the two fits only" in r.stdout
    ids_a, cols, tab_a = hostlib.read_pointwise(base_a + ".pointwise")
    assert ids_a == ["s1", "s2", "s3", "s4"] and cols == list(hostlib.POINTWISE_COLUMNS) and np.isnan(tab_a[1, 6])
    # the other way round: the signs flip
    r = _model_score("--outputFileBase", base_b, "--compareTo", base_a)
    assert r.returncode == 0 and hostlib.read_named_values(base_b + ".modelCompare")["dElpdLoo"] == -want["dElpdLoo"]
    # mismatched ids are refused: another order, another name, another length
    for k, tab in enumerate(([b[1], b[0], b[2], b[3]], [b[0], b[1], ("x3",) + b[2][1:], b[3]], b[:3])):
        with open(tmp_path / f"c{k}.pointwise", "w") as f:
            f.write(header + "".join(" ".join(str(x) for x in line) + "\n" for line in tab))
        r = _model_score("--outputFileBase", base_a, "--compareTo", str(tmp_path / f"c{k}"))
        assert r.returncode != 0 and "differ" in r.stderr
    assert _model_score("--outputFileBase", base_a, "--compareTo", str(tmp_path / "missing")).returncode != 0


def test_short_and_long_flags(host):
    """--perRow / --nPops are modelScore's own spellings of --modelScorePerRow / --modelScoreNPops: both give the same settings,
    on this program's command line only; --perRow takes no value."""
    from cli_util import settings_dump
    short = hostlib.model_score_settings(["--perRow", "--nPops", "2"])
    long_ = hostlib.model_score_settings(["--modelScorePerRow=1", "--modelScoreNPops", "2"])
    assert short == long_ == dict(margIsoIncrem=4, nMassRatios=4, nPops=2, perRow=1, compareTo="")
    assert hostlib.model_score_settings(["--perRow=1", "--nPops=2"]) == short
    assert hostlib.model_score_settings(["--perRow=0"])["perRow"] == 0
    assert settings_dump(["--modelScorePerRow=1", "--modelScoreNPops", "2"]) == {"modelScore.perRow": "1", "modelScore.nPops": "2"}
    assert settings_dump(["--nPops", "2"]) == {"simCluster.nPops": "2"}
    for bad in (["--perRow", "0"], ["--nPops", "2", "--perRow", "0"]):
        with pytest.raises(hostlib.HostError, match="unexpected argument '0'"):
            hostlib.model_score_settings(bad)
    with pytest.raises(hostlib.HostError):
        settings_dump(["--perRow=1"])                                   # no flag of the shared table
    # photResiduals' and massFunction's --perStar is massFunction's key here: accepted, and nothing of modelScore's changes
    assert hostlib.model_score_settings(["--perStar", "--quantity", "system"]) == hostlib.model_score_settings([])
