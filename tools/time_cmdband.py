"""Time b9_cmd_band against the only route the library offered before it, on the same pack and rows in one process: 4096 rows x
8 filters (PARSEC-shaped pack), the loci q = 0 and q = 1 over the pack's whole EEP range, 2 x 512 WD nodes (DA and DB), 30 bins.
Three calls are measured -- the moments call (pivots given), one bins call (first edges), the whole default loop
(hostlib.cmd_band: pivots, moments, first edges, bins passes until every line is final) -- and the old route: per row
b9_derive_isochrone plus ONE b9_predict_mags of all the row's points, then a numpy reduction of the same moments and bins on the
host.  The calls are synchronous; each is bracketed by HIP events (torch.cuda.Event, where torch sees the device) and on the
host (time.perf_counter) -- the whole call, copies included; without a GPU the tool fails.  The new calls are timed before and
after the old route; the old route's host time is split into the two library calls and everything else (numpy, Python).  Prints
one JSON line: medians and all repetitions, the ratios old route / new call, and whether the two routes agree on the MS/RGB
lines (N equal, MIN / MAX within 1e-10; the old route has no node status, so its WD lines are not like for like)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from base_amd import abi, engine, hostlib, synth  # noqa: E402


def events():
    """torch, for its HIP events; a measurement without a device fails here and does not fall back to another clock"""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("time_cmdband: no GPU visible to torch: nothing to measure")
    return torch


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


def old_route(eng, pack_d, rows, eep0, n_eep, ratios, n_nodes, pivot, edges, split=None):
    """(mom, bins) of the same lines (no colours) from b9_derive_isochrone + b9_predict_mags per row and numpy on the host.
    split (a dict, optional): += the host seconds spent inside the two library calls ("calls") and in everything else ("host")."""
    t_calls, t_all0 = 0.0, time.perf_counter()
    nf = pack_d["n_filt"]
    C = 1 + nf
    P = len(ratios) * n_eep + 2 * n_nodes
    n_lines, B = P * C, edges.shape[1] - 1
    mom = np.zeros((n_lines, abi.BAND_NMOM))
    mom[:, abi.BAND_MIN], mom[:, abi.BAND_MAX] = np.inf, -np.inf
    bins = np.zeros((n_lines, B + 3))
    m_up = float(pack_d["m_wd_up"])
    for par in rows:
        t0 = time.perf_counter()
        first, mass, _, tip = eng.derive_isochrone(par, 0)
        t_calls += time.perf_counter() - t0
        v = np.full((P, C), np.nan)
        if len(mass):
            dM = (m_up - tip) / n_nodes
            nodes = tip + dM * np.arange(1, n_nodes + 1)
            m1 = np.concatenate([np.tile(mass, len(ratios)), nodes, nodes])
            q = np.concatenate([np.repeat(ratios, len(mass)), np.zeros(2 * n_nodes)])
            ty = np.concatenate([np.zeros(len(ratios) * len(mass) + n_nodes), np.ones(n_nodes)]).astype(np.int32)
            t0 = time.perf_counter()
            mags, _ = eng.predict_mags(par, m1, q, wd_type=ty)
            t_calls += time.perf_counter() - t0
            mags = np.where(np.isfinite(mags) & (mags != abi.MAG_NOFLUX), mags, np.nan)
            at = np.concatenate([s * n_eep + (first - eep0) + np.arange(len(mass)) for s in range(len(ratios))])
            k = len(at)
            v[at, 0], v[at, 1:] = m1[:k], mags[:k]
            # (the old route has no node status: a node that has not cooled shows its marker magnitude -- counted here as the
            #  call would count a cooled one; the comparison below is made on the MS/RGB lines)
            wd = len(ratios) * n_eep + np.arange(2 * n_nodes)
            ok = nodes <= m_up
            v[wd, 0], v[wd, 1:] = np.where(np.tile(ok, 2), m1[k:], np.nan), np.where(np.tile(ok, 2)[:, None], mags[k:], np.nan)
        v = v.reshape(-1)
        sel = np.flatnonzero(~np.isnan(v))
        d = v[sel] - pivot[sel]
        mom[sel, abi.BAND_N] += 1.0
        mom[sel, abi.BAND_SUM] += d
        mom[sel, abi.BAND_SUMSQ] += d * d
        mom[sel, abi.BAND_MIN] = np.fmin(mom[sel, abi.BAND_MIN], v[sel])
        mom[sel, abi.BAND_MAX] = np.fmax(mom[sel, abi.BAND_MAX], v[sel])
        w = (edges[sel] <= v[sel, None]).sum(axis=1)
        bins[sel, w] += 1.0
        bins[sel, B + 2] += 1.0
    if split is not None:
        split["calls"] = split.get("calls", 0.0) + t_calls
        split["host"] = split.get("host", 0.0) + (time.perf_counter() - t_all0 - t_calls)
    return mom, bins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--wd-nodes", type=int, default=512)
    ap.add_argument("--bins", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--old-reps", type=int, default=3)
    a = ap.parse_args()
    torch = events()
    pack_d = synth.make_pack("parsec", 8)
    truth = synth.default_params(pack_d)
    rows = synth.walker_params(truth, a.rows, seed=3, scale=0.3)
    first, cnt = np.asarray(pack_d["iso_first_eep"]), np.asarray(pack_d["iso_n_eep"])
    eep0, n_eep = int(first.min()), int((first + cnt).max() - first.min())
    ratios = (0.0, 1.0)
    spec = abi.make_band_spec(eep0, n_eep, ratios, a.wd_nodes, 3, ())
    eng = engine.Engine(abi.make_pack(pack_d), None, None, abi.make_options(n_pops=1))
    try:
        n_lines = abi.band_shape(spec.struct, eng.n_filt, 1)[2]
        one, _ = eng.cmd_band(rows[:1], spec)                                        # (also the warm-up)
        pivot = np.where(one[:, abi.BAND_N] > 0, one[:, abi.BAND_MIN], 0.0)
        mom, _ = eng.cmd_band(rows, spec, pivot=pivot)
        edges = hostlib.band_first_edges(mom, a.bins)
        eng.cmd_band(rows[:8], spec, edges=edges, want_mom=False)
        t_mom, (mom, _) = timed(lambda: eng.cmd_band(rows, spec, pivot=pivot), a.reps, torch)
        t_bins, (_, bins) = timed(lambda: eng.cmd_band(rows, spec, edges=edges, want_mom=False), a.reps, torch)
        t_loop, res = timed(lambda: hostlib.cmd_band(eng, rows, spec, n_bins=a.bins), max(1, a.reps // 2), torch)
        old_route(eng, pack_d, rows[:8], eep0, n_eep, ratios, a.wd_nodes, pivot, edges)       # warm-up
        split = {}
        t_old, (mom_o, bins_o) = timed(lambda: old_route(eng, pack_d, rows, eep0, n_eep, ratios, a.wd_nodes, pivot, edges, split), a.old_reps, torch)
        t_old["library_calls_ms_mean"] = 1e3 * split["calls"] / a.old_reps        # host clock around b9_derive_isochrone + b9_predict_mags
        t_old["numpy_and_python_ms_mean"] = 1e3 * split["host"] / a.old_reps
        # the new calls once more AFTER the old route: the two windows of each alternate with it
        t_mom2, _ = timed(lambda: eng.cmd_band(rows, spec, pivot=pivot), a.reps, torch)
        t_bins2, _ = timed(lambda: eng.cmd_band(rows, spec, edges=edges, want_mom=False), a.reps, torch)
    finally:
        eng.close()
    ms = np.arange(len(ratios) * n_eep * (1 + eng.n_filt))                            # the MS/RGB lines
    has = mom[ms, abi.BAND_N] > 0
    agree = bool(np.array_equal(mom[ms, abi.BAND_N], mom_o[ms, abi.BAND_N]) and
                 np.abs(mom[ms][has][:, [abi.BAND_MIN, abi.BAND_MAX]] - mom_o[ms][has][:, [abi.BAND_MIN, abi.BAND_MAX]]).max() <= 1e-10 and
                 np.array_equal(bins[ms][:, -1], bins_o[ms][:, -1]))
    key = "event_ms_median"
    out = dict(tool="time_cmdband", rows=a.rows, n_filt=int(eng.n_filt), eep0=eep0, n_eep=n_eep, ratios=list(ratios), wd_nodes=a.wd_nodes, n_bins=a.bins,
               n_lines=int(n_lines), timed_by="hip events", moments=t_mom, bins=t_bins, moments_after_old=t_mom2, bins_after_old=t_bins2, loop=t_loop,
               loop_passes=int(res["n_passes"]), loop_open_lines=int(((res["flags"] & hostlib.SIV_OPEN) != 0).sum()), old_route=t_old,
               old_over_moments_plus_bins=t_old[key] / (t_mom[key] + t_bins[key]), old_over_loop=t_old[key] / t_loop[key],
               ms_lines_agree=agree, rows_inside=float(mom[:, abi.BAND_N].max()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
