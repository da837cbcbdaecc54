"""Time b9_star_bins, the full default star_intervals loop, b9_mass_hist and the b9_sample_mass route on the same catalogue and
rows in one process: 20k stars (1000 of them WD-stage) x 256 rows x 8 filters (PARSEC-shaped pack) at the 4 x 4 grid by default.
The calls are synchronous, so each is bracketed whole -- the rows' and the edges' upload, the derivation, the node tables, the
kernels, the results' download: by a pair of HIP events (torch.cuda.Event on the null stream) where torch is present, and by the
host clock (time.perf_counter) always.  Prints one JSON line: per call the median and the samples over --reps calls after one
warm-up, one b9_star_bins call at every --bins against b9_mass_hist at 24 bins with row_hist = NULL, the default star_intervals
with its pass count and its share of host time, and b9_sample_mass with the host's quantiles of its draws."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from base_amd import abi, engine, hostlib, synth  # noqa: E402


def events():
    try:
        import torch
        if not torch.cuda.is_available():
            return None
        return torch
    except Exception:
        return None


def timed(fn, reps, torch=None):
    wall, ev, out = [], [], None
    for _ in range(reps):
        if torch is not None:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
        t0 = time.perf_counter()
        out = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        if torch is not None:
            b.record(); b.synchronize()
            ev.append(float(a.elapsed_time(b)))
    return dict(host_ms=wall, host_ms_median=float(np.median(wall)), event_ms=ev, event_ms_median=float(np.median(ev)) if ev else None), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=20000)
    ap.add_argument("--wd-frac", type=float, default=0.05)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--increm", type=int, default=4)
    ap.add_argument("--ratios", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bins", type=int, nargs="+", default=[24, 30])
    ap.add_argument("--quantity", type=int, default=abi.HQ_PRIMARY)
    a = ap.parse_args()
    torch = events()
    pack_d = synth.make_pack("parsec", 8)
    truth = synth.default_params(pack_d)
    cl = synth.make_cluster(pack_d, a.stars, seed=9001, truth=truth, wd_frac=a.wd_frac)
    rows = synth.walker_params(truth, a.rows, seed=3, scale=0.3)
    eng = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cl), synth.default_priors(pack_d, truth),
                        abi.make_options(marg_iso_increm=a.increm, marg_n_q=a.ratios), device=0)
    n = eng.n_stars
    m_up = float(pack_d["m_wd_up"])
    res = dict(stars=n, wd_stage=eng.n_wd_stars(), rows=a.rows, n_filt=8, increm=a.increm, ratios=a.ratios, quantity=a.quantity,
               clock="HIP events and host" if torch is not None else "host")
    edges24 = 0.1 * (m_up / 0.1) ** (np.arange(25) / 24)
    eng.mass_hist(rows[:2], edges24, a.quantity, want_rows=False)          # warm-up: buffers, code object
    res["mass_hist24"], (star, _) = timed(lambda: eng.mass_hist(rows, edges24, a.quantity, want_rows=False), a.reps, torch)
    key = "event_ms_median" if torch is not None else "host_ms_median"
    for nb in a.bins:
        shared = 0.1 * (m_up / 0.1) ** (np.arange(nb + 1) / nb)
        edges = np.tile(shared, (n, 1))
        eng.star_bins(rows[:2], edges, a.quantity)
        t, acc = timed(lambda: eng.star_bins(rows, edges, a.quantity), a.reps, torch)
        t["ratio_to_mass_hist24"] = t[key] / res["mass_hist24"][key]
        if nb == 24:
            t["same_bits_as_mass_hist"] = bool(np.array_equal(acc[:, 1:25], star[:, :24]) and np.array_equal(acc[:, 26], star[:, 24]))
        res[f"star_bins{nb}"] = t
    # the full default loop (its first pass is the warm-up of the 30-bin call above)
    t, out = timed(lambda: hostlib.star_intervals(eng, rows, a.quantity), max(1, a.reps // 2), torch)
    t.update(passes=int(out["n_passes"]), stars_unfinished=int(((out["flags"] & hostlib.SIV_OPEN) != 0).sum()),
             stars_without_mass=int(((out["flags"] & hostlib.SIV_NO_MASS) != 0).sum()), passes_used=np.bincount(out["passes"]).tolist())
    t0 = time.perf_counter()
    hostlib.refine_star_edges(out["edges"], out["acc"])
    t["refine_host_ms_per_pass"] = (time.perf_counter() - t0) * 1e3
    t["ms_per_pass"] = t[key] / t["passes"]
    res["star_intervals"] = t
    # the draws' route: one draw per (row, star), then the host's quantiles of them
    eng.sample_mass(rows[:2], seed=1)
    res["sample_mass"], (mass, ratio, member, pop) = timed(lambda: eng.sample_mass(rows, seed=1), a.reps, torch)
    t0 = time.perf_counter()
    np.quantile(mass, hostlib.STAR_INTERVALS_LEVELS, axis=0)
    res["sample_mass"]["host_quantiles_ms"] = (time.perf_counter() - t0) * 1e3
    res["star_intervals"]["ratio_to_sample_mass"] = res["star_intervals"][key] / res["sample_mass"][key]
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
