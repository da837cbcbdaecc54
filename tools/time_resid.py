"""Time b9_phot_resid against b9_star_moments on the same catalogue and rows in one process: 20k stars (1000 of them
WD-stage) x 256 rows x 8 filters (PARSEC-shaped pack) at the 4 x 4 grid, then 50k stars (--stars takes a list).  The calls are
synchronous, so each is bracketed by HIP events on the null stream (hipEvent through ctypes) and on the host
(time.perf_counter) -- the whole call: the rows' and pivots' upload, the derivation, the node tables,
the kernels, the results' download.  Prints one JSON line per catalogue: median and spread over --reps calls after one
warm-up for both calls, their ratio, and the cost of row_resid (the call with and without it)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from base_amd import abi, engine, synth  # noqa: E402


class HipEvents:
    """hipEvent timing through the HIP runtime itself (ctypes on libamdhip64, the library libbase9hip.so already has loaded):
    events on the null stream around a synchronous call."""

    def __init__(self):
        import ctypes as C
        self.C = C
        self.hip = C.CDLL("libamdhip64.so")

    def _ok(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} returned {rc}")

    def event(self):
        e = self.C.c_void_p()
        self._ok(self.hip.hipEventCreate(self.C.byref(e)), "hipEventCreate")
        return e

    def record(self, e):
        self._ok(self.hip.hipEventRecord(e, None), "hipEventRecord")

    def elapsed_ms(self, a, b):
        self._ok(self.hip.hipEventSynchronize(b), "hipEventSynchronize")
        ms = self.C.c_float()
        self._ok(self.hip.hipEventElapsedTime(self.C.byref(ms), a, b), "hipEventElapsedTime")
        for e in (a, b):
            self.hip.hipEventDestroy(e)
        return float(ms.value)


def timed(fn, reps, ev):
    """(host ms per call, HIP-event ms per call, the last result)"""
    wall, dev, out = [], [], None
    for _ in range(reps):
        a, b = ev.event(), ev.event()
        ev.record(a)
        t0 = time.perf_counter()
        out = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.record(b)
        dev.append(ev.elapsed_ms(a, b))
    return wall, dev, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, nargs="+", default=[20000, 50000])
    ap.add_argument("--wd-frac", type=float, default=0.05)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--filters", type=int, default=8)
    ap.add_argument("--increm", type=int, default=4)
    ap.add_argument("--ratios", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-pruning", action="store_true")
    a = ap.parse_args()
    pack_d = synth.make_pack("parsec", a.filters)
    truth = synth.default_params(pack_d)
    rows = synth.walker_params(truth, a.rows, seed=3, scale=0.3)
    ev = HipEvents()
    for n_stars in a.stars:
        cl = synth.make_cluster(pack_d, n_stars, seed=9001, truth=truth, wd_frac=a.wd_frac)
        eng = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cl), synth.default_priors(pack_d, truth),
                            abi.make_options(marg_iso_increm=a.increm, marg_n_q=a.ratios), device=0)
        if a.no_pruning:
            eng.set_tuning(marg_no_pruning=1)
        n = eng.n_stars
        eng.star_moments(rows[:2])                               # warm-up: buffers, code object
        eng.phot_resid(rows[:2])
        m_wall, m_dev, acc = timed(lambda: eng.star_moments(rows), a.reps, ev)
        r_wall, r_dev, (star, rws) = timed(lambda: eng.phot_resid(rows), a.reps, ev)
        s_wall, s_dev, _ = timed(lambda: eng.phot_resid(rows, want_rows=False), a.reps, ev)
        med, r_med, s_med = float(np.median(m_dev)), float(np.median(r_dev)), float(np.median(s_dev))       # the events' medians
        tie = float(np.max(np.abs(star[:, 1] - acc[:, abi.MOM_MEMBER]) / np.maximum(acc[:, abi.MOM_MEMBER], 1e-300)))
        nf = a.filters
        with np.errstate(invalid="ignore", divide="ignore"):
            chi2 = [float(np.nanmean(rws[:, 3 + 5 * f] / rws[:, 1 + 5 * f])) for f in range(nf)]
        print(json.dumps(dict(
            stars=n, wd_stage=eng.n_wd_stars(), rows=a.rows, n_filt=nf, increm=a.increm, ratios=a.ratios, pruning=not a.no_pruning,
            moments_call_ms=m_wall, moments_call_ms_events=m_dev, moments_call_ms_median=med, moments_ms_per_row=med / a.rows,
            resid_call_ms=r_wall, resid_call_ms_events=r_dev, resid_call_ms_median=r_med, resid_ms_per_row=r_med / a.rows,
            star_rows_per_s=a.rows * n / (r_med * 1e-3), ratio_to_moments=r_med / med,
            without_row_resid_ms_median=s_med, row_resid_cost_ms=r_med - s_med,
            expected_members=float(rws[:, 0].mean()), mean_reduced_chi2_per_filter=chi2, member_against_moments_max_rel=tie)), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
