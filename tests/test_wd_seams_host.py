"""The seam catalogue of the WD branch (tests/wd_seams.py) against its 50-digit reference (tests/wd_ref.py), on the CPU:
coverage of every seam, the budget condition, the C oracle and the numpy restatements at every case, and the power of the
checker against one mutant at a time."""
import math

import numpy as np
import pytest

import oracle
import wd_check
import wd_ref as R
import wd_seams as S
from base_amd import abi, synth

REQUIRED_BRANCHES = {R.DNE, R.BELOW_FIRST, R.MSRGB, R.WD_NOMODELS, R.WD_NOTYET, R.WD, R.NSBH}
REQUIRED_TAGS = {
    "system:no_flux",                                                                                    # a
    "corner:on_tip[0]", "corner:on_tip[1]", "corner:on_tip[na-2]", "corner:on_tip[na-1]",                # b
    "corners:mixed(heavy+inside)", "corners:all_heavy", "corners:mixed(inside+light)", "corner:equal_tips",
    "weidemann:below", "weidemann:node", "weidemann:interior", "weidemann:above", "salaris_pw:low", "salaris_pw:high",   # e
    "wc_mass:below", "wc_mass:node", "wc_mass:interior", "wc_mass:above", "wd_mass:tiny", "wd_mass:nonpositive",
    "wc_age:mixed(below+interior)", "wc_age:mixed(above+interior)", "wc_age:node", "wc_age:two_point_track",   # f
    "wc_age:below", "wc_age:above", "wc_carb:below", "wc_carb:node", "wc_carb:above", "wc_carb:interior",
    "at_teff:below", "at_teff:node", "at_teff:above", "at_logg:below", "at_logg:node", "at_logg:above",  # g
    "atm:DB", "atm:DB_falls_back_to_DA",
}
SIGMA, PRIOR = 0.03125, 0.875


def test_packs_cover_the_shapes():
    P = S.packs()
    shape = lambda k: {(len(d[k]) if k in d else 0) for d, _ in P.values()}
    assert {1, 3} <= shape("y") and {1, 3} <= shape("wc_carb") and {8, 9} <= shape("log_age") and max(shape("log_age")) >= 65
    assert {3, 5, 8} == {d["n_filt"] for d, _ in P.values()}
    assert any("wc_n_age" in d for d, _ in P.values()) and any("wc_mass" in d and "wc_n_age" not in d for d, _ in P.values())
    b = P["B"][0]
    n = b["wc_n_age"].reshape(3, -1)
    assert any(n[i, j] == 2 and n[i, j + 1] >= 65 for i in range(3) for j in range(n.shape[1] - 1))
    assert any(d.get("n_at_type") == 1 for d, _ in P.values()) and any("wc_mass" not in d for d, _ in P.values())
    assert {d.get("ifmr_id") for d, _ in P.values()} >= set(range(6))
    assert all(len(d["iso_n_eep"]) <= 140 and d["iso_n_eep"].max() <= 40 for d, _ in P.values())


def test_coverage_every_seam_is_hit():
    tags, branches = set(), set()
    for c in S.cases():
        tags |= c["ref"]["tags"]
        branches |= set(c["ref"]["branch"])
    assert not REQUIRED_BRANCHES - branches, REQUIRED_BRANCHES - branches
    assert not REQUIRED_TAGS - tags, sorted(REQUIRED_TAGS - tags)
    fams = {c["fam"] for c in S.cases()}
    assert fams == {"a", "b", "c", "d", "e", "f", "g", "NaN"}
    # c: both sides of prec >= logAge next to each other, above the tip; d: the five distances
    for c in S.cases():
        if c["fam"] == "c":
            assert c["ref"]["branch"][0] in (R.WD, R.WD_NOTYET)
    assert {R.WD, R.WD_NOTYET} == {c["ref"]["branch"][0] for c in S.cases() if c["fam"] == "c"}
    on = [c for c in S.cases() if c["fam"] == "c" and c["ref"].get("prec") is not None
          and c["ref"]["prec"].v == S.packs()[c["pack"]][1][c["row"]][abi.P_LOGAGE]]
    assert on and all(c["ref"]["branch"] == [R.WD_NOTYET] for c in on), "no case with prec == logAge exactly, above the tip"
    assert sorted({c["ulps"] for c in S.cases() if c["fam"] == "d"}) == [1, 2, 16, 1000, 10 ** 6]
    for c in S.cases():
        if c["fam"] == "d":                       # prec is the grid age exactly; logAge the stated number of ulps above it
            la = S.packs()[c["pack"]][1][c["row"]][abi.P_LOGAGE]
            assert c["ref"]["branch"] == [R.WD] and float(c["ref"]["prec"].v) + c["ulps"] * math.ulp(la) == la
    # WD primary with an MS companion
    assert any(c["ref"]["branch"] == [R.WD, R.MSRGB] for c in S.cases())
    weak = [c for c in S.cases() if c["fam"] in S.WEAK]
    print(f"{len(S.cases())} cases, {len(weak)} weak (families d and NaN)")


def test_budget_condition_outside_the_weak_families():
    """kappa u <= 2^-10 and budget <= 1e-9 max(1, |value|) for every quantity of every case outside families d and NaN: the
    budget cannot hide a failure of the project's parity tolerance."""
    worst = 0.0
    for c in S.cases():
        if c["fam"] in S.WEAK:
            continue
        assert S.meets_budget(c["ref"]), (c["fam"], c["pack"], c["row"], c["m1"])
        if c["ref"].get("kappa") is not None:
            worst = max(worst, float(c["ref"]["kappa"]))
    print(f"largest kappa outside the weak families: {worst:.3g}")
    assert all(c["fam"] == "NaN" for c in S.cases() if any(isinstance(a, str) for a in c["ref"].get("app_mags") or []))


def _f64(c, mut=None, cache={}):
    d, rows = S.packs()[c["pack"]]
    key = (c["pack"], c["row"], c["pop"], mut)
    if key not in cache:
        cache[key] = R.Model(R.F64, d, rows[c["row"]], c["pop"], mut)
    return R.evaluate(d, rows[c["row"]], c["pop"], c["m1"], c["q"], c["wd_type"], B=R.F64, mut=mut, model=cache[key])


def _rejects(c, got):
    """the checker: does the result `got` (an F64 evaluation) of case c fail against the reference?"""
    if got["branch"] != c["ref"]["branch"]:
        return True
    return S.mag_ratio(c, [abi.MAG_NOFLUX if a is None else (math.nan if isinstance(a, str) else a) for a in got["app_mags"]]) > 1.0


def test_fp64_emulation_passes_at_every_case():
    worst = {}
    for c in S.cases():
        got = _f64(c)
        assert got["branch"] == c["ref"]["branch"], (c["fam"], c["pack"], c["row"], c["m1"])
        r = S.mag_ratio(c, [abi.MAG_NOFLUX if a is None else (math.nan if isinstance(a, str) else a) for a in got["app_mags"]])
        assert r <= 1.0, (c["fam"], c["pack"], c["row"], c["m1"], r)
        worst[c["fam"]] = max(worst.get(c["fam"], 0.0), r)
    print("fp64 emulation, |emulation - reference| / tolerance per family:", {k: round(v, 4) for k, v in sorted(worst.items())})


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_checker_rejects_mutant(mut):
    strong = [c for c in S.cases() if c["fam"] not in S.WEAK]
    assert any(_rejects(c, _f64(c, mut)) for c in strong), f"no case of the catalogue notices the mutant {mut}"


def test_oracle_agrees_with_the_reference_at_every_case():
    """b9o_logpost(perstar) at the reference's magnitudes + known offsets: the per-star mixture value within the propagated
    tolerance; the NaN family gives the field-only value.  (The oracle forms the flux sum with two pow and a log10 where the
    reference states the device's log1pexp form; the two differ by a few ulp of the magnitude, inside the budget's 4e-16.)"""
    worst, n = {}, 0
    for name, (d, rows) in S.packs().items():
        pack = abi.make_pack(d)
        for irow, (cl, cs) in S.catalogue(name, prior=PRIOR, sigma=SIGMA).items():
            stars = abi.make_stars(cl)
            o = oracle.Oracle(pack, stars, abi.make_priors(), abi.make_options())
            _, ps = o.logpost(rows[irow][None, :], perstar=True)
            for c, got in zip(cs, ps[0]):
                want = S.like(name, c, SIGMA, PRIOR)["value"]
                r = S.value_ratio(want, got)
                assert math.isfinite(got) and r <= 1.0, (c["fam"], name, irow, c["m1"], c["q"], got, want and float(want.v), r)
                worst[c["fam"]] = max(worst.get(c["fam"], 0.0), r)
                n += 1
    print(f"oracle at {n} cases, |oracle - reference| / tolerance per family:", {k: round(v, 4) for k, v in sorted(worst.items())})


def test_numpy_restatements_agree_with_the_reference():
    """wd_check.wd_chain's intermediates and synth.forward_mags' magnitudes at every case of their domain.  Outside it, written
    down rather than bent: (1) synth._ifmr clamps Weidemann's table with np.interp where the model extrapolates -- forward_mags is
    compared on Weidemann packs only for 1 <= m <= 7 (wd_check.ifmr extrapolates and is compared everywhere); (2) both invert a
    tip column with np.interp, which needs strictly monotone nodes -- masses on or next to the two equal tips are left to the
    oracle; (3) both clamp 10^logAge - 10^prec at 1e-300, which only differs from the model where prec >= logAge, and there both
    overwrite the result as the model does; (4) wd_mass <= 0 gives NaN in numpy as well (compared as not finite); (5) a system
    without flux is not B9_MAG_NOFLUX in forward_mags (it adds two fluxes of magnitude 99.999): b9_predict_mags' rule only."""
    worst = {}
    for c in S.cases():
        d, rows = S.packs()[c["pack"]]
        ref, row = c["ref"], rows[c["row"]]
        if not ref["model"].valid or not c["m1"] > 0 or "corner:equal_tips" in ref["tags"]:
            continue
        weide_out = d.get("ifmr_id") == abi.IFMR_WEIDEMANN and not 1.0 <= c["m1"] <= 7.0
        with np.errstate(all="ignore"):
            if ref["branch"][0] in (R.WD, R.WD_NOTYET):
                got = wd_check.wd_chain(d, row, [c["m1"]], c["pop"])
                names = ("wd_mass", "prec") + (("log_cool", "log_teff", "logg") if ref["branch"][0] == R.WD else ())
                for k, g in zip(("wd_mass", "prec", "log_cool", "log_teff", "logg"), got):
                    if k in names and c["fam"] != "NaN":
                        r = S.value_ratio(ref[k], float(g[0]))
                        assert r <= 1.0, (k, c["fam"], c["pack"], c["row"], c["m1"], float(g[0]), float(ref[k].v), r)
                        worst[k] = max(worst.get(k, 0.0), r)
            if weide_out or "system:no_flux" in ref["tags"]:
                continue
            mags = synth.forward_mags(d, row, [c["m1"]], [c["q"]], [c["wd_type"]], pop=c["pop"])[0]
        want = dict(c, ref=dict(ref, app_mags=ref["like_mags"]))
        r = S.mag_ratio(want, mags)
        assert r <= 1.0, (c["fam"], c["pack"], c["row"], c["m1"], c["q"], r)
        worst["mags " + c["fam"]] = max(worst.get("mags " + c["fam"], 0.0), r)
    print("numpy restatements, |numpy - reference| / tolerance:", {k: round(v, 4) for k, v in sorted(worst.items())})
