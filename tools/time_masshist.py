"""Time b9_mass_hist against b9_star_moments on the same catalogue and rows in one process: 20k stars (1000 of them
WD-stage) x 256 rows x 8 filters (PARSEC-shaped pack) at the 4 x 4 grid by default, 24 and 64 log-spaced bins of the primary
mass over [0.1, M_wd_up].  The calls are synchronous, so each is bracketed on the host (time.perf_counter) -- the whole call:
the rows' upload, the derivation, the node tables, the kernels, the results' download.  Prints one JSON line: median and
spread over --reps calls after one warm-up for both calls, their ratio per bin count, and the cost of row_hist (the call
with and without it)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from base_amd import abi, engine, synth  # noqa: E402


def timed(fn, reps):
    wall, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
    return wall, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=20000)
    ap.add_argument("--wd-frac", type=float, default=0.05)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--increm", type=int, default=4)
    ap.add_argument("--ratios", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bins", type=int, nargs="+", default=[24, 64])
    ap.add_argument("--quantity", type=int, default=abi.HQ_PRIMARY)
    ap.add_argument("--no-pruning", action="store_true")
    a = ap.parse_args()
    pack_d = synth.make_pack("parsec", 8)
    truth = synth.default_params(pack_d)
    cl = synth.make_cluster(pack_d, a.stars, seed=9001, truth=truth, wd_frac=a.wd_frac)
    rows = synth.walker_params(truth, a.rows, seed=3, scale=0.3)
    eng = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cl), synth.default_priors(pack_d, truth),
                        abi.make_options(marg_iso_increm=a.increm, marg_n_q=a.ratios), device=0)
    if a.no_pruning:
        eng.set_tuning(marg_no_pruning=1)
    n = eng.n_stars
    m_up = float(pack_d["m_wd_up"])
    eng.star_moments(rows[:2])                               # warm-up: buffers, code object
    wall, acc = timed(lambda: eng.star_moments(rows), a.reps)
    med = float(np.median(wall))
    res = dict(stars=n, wd_stage=eng.n_wd_stars(), rows=a.rows, n_filt=8, increm=a.increm, ratios=a.ratios, pruning=not a.no_pruning,
               quantity=a.quantity, moments_call_ms=wall, moments_call_ms_median=med, moments_ms_per_row=med / a.rows)
    for nb in a.bins:
        edges = 0.1 * (m_up / 0.1) ** (np.arange(nb + 1) / nb)
        eng.mass_hist(rows[:2], edges, a.quantity)
        h_wall, (star, rws) = timed(lambda: eng.mass_hist(rows, edges, a.quantity), a.reps)
        s_wall, _ = timed(lambda: eng.mass_hist(rows, edges, a.quantity, want_rows=False), a.reps)
        h_med, s_med = float(np.median(h_wall)), float(np.median(s_wall))
        tie = float(np.max(np.abs(star[:, nb] - acc[:, abi.MOM_MEMBER]) / np.maximum(acc[:, abi.MOM_MEMBER], 1e-300)))
        res[f"hist{nb}"] = dict(call_ms=h_wall, call_ms_median=h_med, ms_per_row=h_med / a.rows, star_rows_per_s=a.rows * n / (h_med * 1e-3),
                                ratio_to_moments=h_med / med, without_row_hist_ms_median=s_med, row_hist_cost_ms=h_med - s_med,
                                expected_members_in_range=float(rws[:, :nb].sum(axis=1).mean()), expected_members=float(rws[:, nb].mean()),
                                total_column_against_moments_member_max_rel=tie)
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
