"""Time b9_filter_loo against b9_phot_resid and against the route the library had before -- the catalogue reloaded n_filt times
with one band's sigma set to -1, each reload followed by b9_phot_resid and a marginalised per-star b9_logpost -- on the same
catalogue and rows in one process: 20k stars (1000 of them WD-stage) x 256 rows x 8 filters (PARSEC-shaped pack) at the 4 x 4
grid (--stars takes a list).  The calls are synchronous, so each is bracketed by HIP events on the null stream and on the host
(tools/time_resid.py's HipEvents) -- the whole call, copies included.  Prints one JSON line per catalogue: medians over --reps
calls after one warm-up of b9_filter_loo with and without the row sums, of b9_phot_resid, and of the reload route as a whole
(--reload-reps of it: it is the slow one), and the ratios."""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reload-reps", type=int, default=2)
    ap.add_argument("--no-pruning", action="store_true")
    a = ap.parse_args()
    pack_d = synth.make_pack("parsec", a.filters)
    truth = synth.default_params(pack_d)
    rows = synth.walker_params(truth, a.rows, seed=3, scale=0.3)
    ev = HipEvents()
    nf = a.filters
    for n_stars in a.stars:
        cl = synth.make_cluster(pack_d, n_stars, seed=9001, truth=truth, wd_frac=a.wd_frac)
        full = abi.make_stars(cl)
        less = []
        for f in range(nf):
            cf = dict(cl)
            cf["sigma"] = np.array(cl["sigma"], dtype=np.float64)
            cf["sigma"][:, f] = -1.0
            less.append(abi.make_stars(cf))
        eng = engine.Engine(abi.make_pack(pack_d), full, synth.default_priors(pack_d, truth),
                            abi.make_options(mode=abi.MODE_MARGINALISED, marg_iso_increm=a.increm, marg_n_q=a.ratios), device=0)
        if a.no_pruning:
            eng.set_tuning(marg_no_pruning=1)
        n = eng.n_stars
        eng.phot_resid(rows[:2])                                 # warm-up: buffers, code object
        eng.filter_loo(rows[:2])
        eng.logpost(rows[:2], perstar=True)
        l_wall, l_dev, (star, rws) = timed(lambda: eng.filter_loo(rows), a.reps, ev)
        s_wall, s_dev, _ = timed(lambda: eng.filter_loo(rows, want_rows=False), a.reps, ev)
        r_wall, r_dev, (res, _) = timed(lambda: eng.phot_resid(rows), a.reps, ev)

        def reload_route():
            out = None
            for f in range(nf):
                eng.load_stars(less[f])
                out = eng.phot_resid(rows, want_rows=False)
                eng.logpost(rows, perstar=True)
            return out

        o_wall, o_dev, _ = timed(reload_route, a.reload_reps, ev)
        eng.close()
        l_med, s_med, r_med, o_med = (float(np.median(v)) for v in (l_dev, s_dev, r_dev, o_dev))
        tie = float(np.max(np.abs(star[:, 1] - res[:, 1]) / np.maximum(res[:, 1], 1e-300)))
        with np.errstate(invalid="ignore", divide="ignore"):
            chi2 = [float(np.nanmean(rws[:, 3 + 6 * f] / rws[:, 1 + 6 * f])) for f in range(nf)]
            lpd = [float(np.nanmean(rws[:, 6 + 6 * f] / rws[:, 1 + 6 * f])) for f in range(nf)]
        print(json.dumps(dict(
            stars=n, rows=a.rows, n_filt=nf, increm=a.increm, ratios=a.ratios, pruning=not a.no_pruning,
            loo_call_ms_events=l_dev, loo_call_ms=l_wall, loo_call_ms_median=l_med, loo_ms_per_row=l_med / a.rows,
            star_rows_per_s=a.rows * n / (l_med * 1e-3),
            loo_without_row_sums_ms_median=s_med, row_sums_cost_ms=l_med - s_med,
            resid_call_ms_events=r_dev, resid_call_ms_median=r_med, ratio_to_resid=l_med / r_med,
            reload_route_ms_events=o_dev, reload_route_ms=o_wall, reload_route_ms_median=o_med, reload_route_over_loo=o_med / l_med,
            mean_loo_reduced_chi2_per_filter=chi2, mean_lpd_per_filter=lpd, member_against_resid_max_rel=tie)), flush=True)


if __name__ == "__main__":
    main()
