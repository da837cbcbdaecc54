"""Time b9_star_offset against b9_phot_resid and b9_filter_loo on the same catalogue and rows in one process: 20k stars (1000 of
them WD-stage) x 256 rows x 8 filters (PARSEC-shaped pack) at the 4 x 4 grid (--stars takes a list).  The calls are synchronous,
so each is bracketed by HIP events on the null stream and on the host (tools/time_resid.py's HipEvents) -- the whole call,
copies included.  Prints one JSON line per catalogue: medians over --reps calls (20) after one warm-up of b9_star_offset with
one direction (absorption) and with two (absorption, distance), per-star output only and with the row sums, of b9_phot_resid
and of b9_filter_loo, the ratios, and the same calls with b9_tuning.marg_no_pruning -- the offset call's time with the pruning
over its time without is what share of the node table its walk still evaluates, next to the same ratio of the full-data walk
(b9_phot_resid)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from base_amd import abi, engine, synth  # noqa: E402
from time_resid import HipEvents, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, nargs="+", default=[20000])
    ap.add_argument("--wd-frac", type=float, default=0.05)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--filters", type=int, default=8)
    ap.add_argument("--increm", type=int, default=4)
    ap.add_argument("--ratios", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tau", type=float, default=0.1)
    a = ap.parse_args()
    pack_d = synth.make_pack("parsec", a.filters)
    truth = synth.default_params(pack_d)
    rows = synth.walker_params(truth, a.rows, seed=3, scale=0.3)
    ev = HipEvents()
    nf = a.filters
    k2 = np.stack([np.asarray(pack_d["abs_coeff"], dtype=np.float64)[:nf], np.ones(nf)])
    for n_stars in a.stars:
        cl = synth.make_cluster(pack_d, n_stars, seed=9001, truth=truth, wd_frac=a.wd_frac)
        eng = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cl), synth.default_priors(pack_d, truth),
                            abi.make_options(mode=abi.MODE_MARGINALISED, marg_iso_increm=a.increm, marg_n_q=a.ratios), device=0)
        n = eng.n_stars
        eng.phot_resid(rows[:2])                                 # warm-up: buffers, code object
        eng.filter_loo(rows[:2])
        eng.star_offset(rows[:2], k2, a.tau)
        eng.star_offset(rows[:2], k2[:1], a.tau)

        def med(fn):
            _, dev, out = timed(fn, a.reps, ev)
            return float(np.median(dev)), out

        out = dict(stars=n, rows=a.rows, n_filt=nf, increm=a.increm, ratios=a.ratios, tau=a.tau, reps=a.reps)
        for tag, tuning in (("", {}), ("_unpruned", {"marg_no_pruning": 1})):
            eng.set_tuning(**tuning)
            out["off_d1_star_ms" + tag], _ = med(lambda: eng.star_offset(rows, k2[:1], a.tau, want_rows=False))
            out["off_d1_ms" + tag], _ = med(lambda: eng.star_offset(rows, k2[:1], a.tau))
            out["off_d2_star_ms" + tag], (star, _) = med(lambda: eng.star_offset(rows, k2, a.tau, want_rows=False))
            out["off_d2_ms" + tag], (_, rws) = med(lambda: eng.star_offset(rows, k2, a.tau))
            out["resid_ms" + tag], (res, _) = med(lambda: eng.phot_resid(rows))
            out["loo_ms" + tag], _ = med(lambda: eng.filter_loo(rows))
            out["loo_star_ms" + tag], _ = med(lambda: eng.filter_loo(rows, want_rows=False))
            if not tag:
                out["member_against_resid_equal"] = bool(np.array_equal(star[:, :2], res[:, :2]))
                with np.errstate(invalid="ignore", divide="ignore"):
                    out["mean_offset_per_direction"] = [float(np.nanmean(rws[:, 2 + 4 * j] / rws[:, 1 + 4 * j])) for j in range(2)]
                    out["mean_logBF_per_direction"] = [float(np.nanmean(rws[:, 4 + 4 * j] / rws[:, 1 + 4 * j])) for j in range(2)]
        eng.set_tuning()
        eng.close()
        out.update(
            star_rows_per_s_d2=a.rows * n / (out["off_d2_ms"] * 1e-3),
            row_sums_cost_ms_d1=out["off_d1_ms"] - out["off_d1_star_ms"], row_sums_cost_ms_d2=out["off_d2_ms"] - out["off_d2_star_ms"],
            d1_over_resid=out["off_d1_ms"] / out["resid_ms"], d2_over_resid=out["off_d2_ms"] / out["resid_ms"],
            d1_over_loo=out["off_d1_ms"] / out["loo_ms"], d2_over_loo=out["off_d2_ms"] / out["loo_ms"],
            d1_star_over_loo_star=out["off_d1_star_ms"] / out["loo_star_ms"], d2_star_over_loo_star=out["off_d2_star_ms"] / out["loo_star_ms"],
            d2_over_d1=out["off_d2_ms"] / out["off_d1_ms"],
            share_evaluated_offset_d1=out["off_d1_star_ms"] / out["off_d1_star_ms_unpruned"],
            share_evaluated_offset_d2=out["off_d2_star_ms"] / out["off_d2_star_ms_unpruned"],
            share_evaluated_full_data=out["resid_ms"] / out["resid_ms_unpruned"],
            share_evaluated_loo=out["loo_star_ms"] / out["loo_star_ms_unpruned"])
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
