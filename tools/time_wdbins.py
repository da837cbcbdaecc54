"""Time b9_wd_bins next to b9_wd_moments and b9_sample_wd_mass on the same rows and nodes, in the same run: 20k stars (1000
WD-stage) x 8 filters (PARSEC-shaped pack), 256 rows, 512 nodes.  HIP events (torch.cuda.Event) around each synchronous call --
the whole call, copies included -- with the host's clock next to them (tools/time_wdmoments.py's timed).  Measures one quantity
at 24 and at 30 bins, all six at 30 bins, six one-quantity calls at 30 bins, b9_wd_moments as the yardstick, the full default
hostlib.wd_intervals loop with its pass count, and sample_wd_mass plus host quantiles of the same rows.  Prints one JSON line:
medians and spreads over --reps calls after one warm-up, and the ratios."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from base_amd import abi, engine, hostlib, synth  # noqa: E402
from time_wdmoments import timed  # noqa: E402


def stats(ms):
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=20000)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--nodes", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--wd-frac", type=float, default=0.05)
    a = ap.parse_args()
    pack_d = synth.make_pack("parsec", 8)
    truth = synth.default_params(pack_d)
    rows = synth.walker_params(truth, a.rows, seed=3, scale=0.3)
    cl = synth.make_cluster(pack_d, a.stars, seed=9001, truth=truth, wd_frac=a.wd_frac)
    eng = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cl), synth.default_priors(pack_d, truth), abi.make_options(), device=0)
    n_wd = eng.n_wd_stars()
    res = {}
    # edges: every line's first range of the default loop, cut evenly
    lo, hi = hostlib.wd_first_ranges(eng.wd_moments(rows, a.nodes)[0])

    def edges_of(n_bins, qs):
        return np.ascontiguousarray(lo[:, qs, None] + (hi - lo)[:, qs, None] * (np.arange(n_bins + 1) / n_bins))

    def mask_of(qs):
        return sum(1 << q for q in qs)

    out = dict(stars=a.stars, wd_stage=n_wd, rows=a.rows, nodes=a.nodes, n_filt=8, reps=a.reps)
    ev, host, clock = timed(lambda: res.update(mom=eng.wd_moments(rows, a.nodes)[0]), a.reps)
    out.update(clock=clock, wd_moments_ms=stats(ev))
    for name, n_bins, qs in (("one_quantity_24_bins", 24, [abi.WQ_LOGCOOL]), ("one_quantity_30_bins", 30, [abi.WQ_LOGCOOL]),
                             ("six_quantities_30_bins", 30, list(range(6)))):
        e = edges_of(n_bins, qs)
        ev, host, _ = timed(lambda: res.update(acc=eng.wd_bins(rows, a.nodes, e, mask_of(qs))[0]), a.reps)
        out[name + "_ms"] = stats(ev)
    singles = [edges_of(30, [q]) for q in range(6)]

    def six_calls():
        for q in range(6):
            eng.wd_bins(rows, a.nodes, singles[q], 1 << q)
    ev, host, _ = timed(six_calls, a.reps)
    out["six_one_quantity_calls_30_bins_ms"] = stats(ev)
    ev, host, _ = timed(lambda: res.update(iv=hostlib.wd_intervals(eng, rows, a.nodes)), max(2, a.reps // 2))
    out["wd_intervals_loop_ms"] = stats(ev)
    out["wd_intervals_passes"] = int(res["iv"]["n_passes"])
    out["wd_intervals_lines_open"] = int(np.sum((res["iv"]["flags"] & hostlib.SIV_OPEN) != 0))
    out["wd_intervals_passes_used"] = np.bincount(res["iv"]["passes"]).tolist()

    def draws_and_quantiles():
        g = eng.sample_wd_mass(rows, a.nodes, seed=1)
        res.update(q=[np.quantile(g[k], hostlib.STAR_INTERVALS_LEVELS, axis=0) for k in ("zams", "wd_mass", "prec_log_age", "log_cool_age", "log_teff", "logg")])
    ev, host, _ = timed(draws_and_quantiles, a.reps)
    out["sample_wd_mass_plus_quantiles_ms"] = stats(ev)
    med = lambda k: out[k]["median"]      # noqa: E731
    out["ratio_one_quantity_30_to_wd_moments"] = med("one_quantity_30_bins_ms") / med("wd_moments_ms")
    out["ratio_six_quantities_to_wd_moments"] = med("six_quantities_30_bins_ms") / med("wd_moments_ms")
    out["ratio_six_quantities_to_six_calls"] = med("six_quantities_30_bins_ms") / med("six_one_quantity_calls_30_bins_ms")
    out["ratio_loop_to_draws_and_quantiles"] = med("wd_intervals_loop_ms") / med("sample_wd_mass_plus_quantiles_ms")
    out["node_evals_per_s_six_quantities"] = a.rows * n_wd * a.nodes * 6 / (med("six_quantities_30_bins_ms") * 1e-3)
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
