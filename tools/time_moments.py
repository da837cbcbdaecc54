"""Time b9_star_moments against the only other route to a per-star summary, b9_sample_mass + a host average of its draws, on
the same catalogue and rows in one run: 20k stars (1000 of them WD-stage) x 256 rows x 8 filters (PARSEC-shaped pack) at the
4 x 4 grid by default.  The calls are synchronous, so each is bracketed on the host (time.perf_counter) and, as a cross-check,
by HIP events on the default stream (torch.cuda.Event; left out where torch cannot open the device) -- the whole call: the rows' upload, the derivation, the node tables,
the kernels, the results' download.  Prints one JSON line: median and spread over --reps calls after one warm-up, ms per row
and star-rows per second for both routes, and the host time to average the draws."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from base_amd import abi, engine, synth  # noqa: E402


def timed(fn, reps):
    """(host ms per call, event ms per call or [] where torch cannot open the device, the last result)"""
    try:
        import torch
        torch.cuda.init()
        event = lambda: torch.cuda.Event(enable_timing=True)      # noqa: E731
    except Exception:                                              # the figures that count are the host's: the calls are synchronous
        event = None
    wall, dev, out = [], [], None
    for _ in range(reps):
        if event:
            a, b = event(), event()
            a.record()
        t0 = time.perf_counter()
        out = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        if event:
            b.record()
            b.synchronize()
            dev.append(a.elapsed_time(b))
    return wall, dev, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=20000)
    ap.add_argument("--wd-frac", type=float, default=0.05)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--increm", type=int, default=4)
    ap.add_argument("--ratios", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
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
    eng.star_moments(rows[:2])                               # warm-up: buffers, code object
    eng.sample_mass(rows[:2], seed=1)
    wall, dev, acc = timed(lambda: eng.star_moments(rows), a.reps)
    s_wall, s_dev, draws = timed(lambda: eng.sample_mass(rows, seed=1), a.reps)
    t0 = time.perf_counter()
    mass, ratio, member, pop = draws
    w = member.sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_drawn = (member * mass).sum(axis=0) / w
    avg_ms = (time.perf_counter() - t0) * 1e3
    tab = engine.star_table(acc)
    ok = (w > 0) & (tab[:, 1] > 0.5)
    med, s_med = float(np.median(wall)), float(np.median(s_wall))
    print(json.dumps(dict(
        stars=n, wd_stage=eng.n_wd_stars(), rows=a.rows, n_filt=8, increm=a.increm, ratios=a.ratios, pruning=not a.no_pruning,
        moments_call_ms=wall, moments_call_ms_median=med, moments_event_ms_median=float(np.median(dev)) if dev else None,
        moments_ms_per_row=med / a.rows, moments_star_rows_per_s=a.rows * n / (med * 1e-3),
        sample_mass_call_ms=s_wall, sample_mass_call_ms_median=s_med, sample_mass_event_ms_median=float(np.median(s_dev)) if s_dev else None,
        sample_mass_ms_per_row=s_med / a.rows, sample_mass_star_rows_per_s=a.rows * n / (s_med * 1e-3),
        host_average_ms=avg_ms, rows_counted_min=float(acc[:, 0].min()), rows_counted_max=float(acc[:, 0].max()),
        median_abs_mass_difference_to_averaged_draws=float(np.median(np.abs(mean_drawn[ok] - tab[ok, 2]))))))
    eng.close()


if __name__ == "__main__":
    main()
