"""Time b9_wd_moments next to b9_sample_wd_mass on the same rows and nodes, in the same run: 20k stars x 8 filters
(PARSEC-shaped pack), 256 rows, 512 nodes, once with 5 % of the stars WD-stage (1000) and once with 0.1 % (20).  HIP events
(torch.cuda.Event) around each synchronous call -- the whole call, copies included: the rows' upload, the derivation, the
table, the star kernel, the accumulation, the results' download -- with the host's clock next to them.  Prints one JSON line
per shape: median and spread over --reps calls after one warm-up, node evaluations per second, and the ratio of the two calls."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from base_amd import abi, engine, synth  # noqa: E402


def timed(call, reps):
    """(event ms, host ms, which clock the first is) of `reps` calls after one warm-up (buffers, code object); where torch cannot open the device the
    host's clock stands in for the events."""
    try:
        import torch
        events = torch.cuda.is_available()
    except Exception:
        events = False
    call()
    ev_ms, host_ms = [], []
    for _ in range(reps):
        if events:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
        t0 = time.perf_counter()
        call()
        host_ms.append((time.perf_counter() - t0) * 1e3)
        if events:
            e1.record()
            e1.synchronize()
            ev_ms.append(float(e0.elapsed_time(e1)))
    return (ev_ms if events else list(host_ms)), host_ms, ("hip events" if events else "host")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=20000)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--nodes", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--wd-frac", type=float, nargs="+", default=[0.05, 0.001])
    a = ap.parse_args()
    pack_d = synth.make_pack("parsec", 8)
    truth = synth.default_params(pack_d)
    rows = synth.walker_params(truth, a.rows, seed=3, scale=0.3)
    for frac in a.wd_frac:
        cl = synth.make_cluster(pack_d, a.stars, seed=9001, truth=truth, wd_frac=frac)
        eng = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cl), synth.default_priors(pack_d, truth), abi.make_options(), device=0)
        n_wd = eng.n_wd_stars()
        res = {}
        mom_ev, mom_host, clock = timed(lambda: res.update(acc=eng.wd_moments(rows, a.nodes)[0]), a.reps)
        smp_ev, smp_host, _ = timed(lambda: res.update(g=eng.sample_wd_mass(rows, a.nodes, seed=1)), a.reps)
        med, med_s = float(np.median(mom_ev)), float(np.median(smp_ev))
        print(json.dumps(dict(stars=a.stars, wd_stage=n_wd, rows=a.rows, nodes=a.nodes, n_filt=8, clock=clock,
                              wd_moments_ms_median=med, wd_moments_ms_min=float(min(mom_ev)), wd_moments_ms_max=float(max(mom_ev)),
                              wd_moments_host_ms_median=float(np.median(mom_host)),
                              sample_wd_mass_ms_median=med_s, sample_wd_mass_ms_min=float(min(smp_ev)), sample_wd_mass_ms_max=float(max(smp_ev)),
                              sample_wd_mass_host_ms_median=float(np.median(smp_host)),
                              ratio=med / med_s, node_evals_per_s=a.rows * n_wd * a.nodes / (med * 1e-3),
                              rows_counted=float(res["acc"][:, abi.WDM_ROWS].sum()), drawn=int(np.sum(res["g"]["zams"] > 0)))))
        eng.close()


if __name__ == "__main__":
    main()
