"""Time b9_pointwise against b9_star_moments on the same catalogue and rows in one process: 20k stars (1000 of them
WD-stage) x 256 rows x 8 filters (PARSEC-shaped pack) at the 4 x 4 grid, then 50k stars (--stars takes a list).  The calls are
synchronous, so each is bracketed by HIP events on the null stream (hipEvent through ctypes) and on the host
(time.perf_counter) -- the whole call: the rows' upload, the derivation, the node tables, the kernels, the results' download.
Prints one JSON line per catalogue: median and spread over --reps calls after one warm-up for b9_star_moments and for
b9_pointwise with tail_len = --tail (49: what modelScore picks for 256 rows), with tail_len = 0, and with acc alone
(no tail, no row sums); the ratios to b9_star_moments."""
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
    ap.add_argument("--tail", type=int, default=49)
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
        eng.pointwise(rows[:2], a.tail)
        m_wall, m_dev, mom = timed(lambda: eng.star_moments(rows), a.reps, ev)
        t_wall, t_dev, (acc, tail, lpd) = timed(lambda: eng.pointwise(rows, a.tail), a.reps, ev)
        z_wall, z_dev, _ = timed(lambda: eng.pointwise(rows, 0), a.reps, ev)
        o_wall, o_dev, _ = timed(lambda: eng.pointwise(rows, 0, want_rows=False), a.reps, ev)
        med, t_med, z_med, o_med = (float(np.median(x)) for x in (m_dev, t_dev, z_dev, o_dev))       # the events' medians
        print(json.dumps(dict(
            stars=n, wd_stage=eng.n_wd_stars(), rows=a.rows, n_filt=a.filters, increm=a.increm, ratios=a.ratios, pruning=not a.no_pruning,
            tail_len=a.tail, moments_call_ms=m_wall, moments_call_ms_events=m_dev, moments_call_ms_median=med,
            pointwise_call_ms=t_wall, pointwise_call_ms_events=t_dev, pointwise_call_ms_median=t_med, ratio_to_moments=t_med / med,
            no_tail_call_ms_events=z_dev, no_tail_call_ms_median=z_med, no_tail_ratio_to_moments=z_med / med,
            acc_only_call_ms_events=o_dev, acc_only_call_ms_median=o_med, acc_only_ratio_to_moments=o_med / med,
            tail_cost_ms=t_med - z_med, row_lpd_cost_ms=z_med - o_med, star_rows_per_s=a.rows * n / (t_med * 1e-3),
            rows_counted=float(acc[:, abi.PW_ROWS].mean()), stars_with_minus_inf=int((acc[:, abi.PW_NINF] > 0).sum()),
            mean_row_lpd_per_star=float(np.mean(lpd[np.isfinite(lpd)]) / n), tail_filled=float(np.isfinite(tail).mean()),
            rows_against_moments_equal=bool(np.array_equal(acc[:, abi.PW_ROWS] >= mom[:, abi.MOM_ROWS], np.ones(n, bool))))), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
