"""Time b9_ratio_hist against b9_mass_hist(PRIMARY) at the same number of columns, on the same catalogue and rows in one process:
20k stars (1000 of them WD-stage) x 256 rows x 8 filters (PARSEC-shaped pack), the 4 x 4 and the 8 x 8 grid, 8 log-spaced bins
of the primary mass over [0.1, M_wd_up] -- 32 and 64 cells, against b9_mass_hist at 32 and 64 bins over the same range.  The
calls are synchronous; each is bracketed by HIP events (torch.cuda.Event, where torch sees the device) and on the host
(time.perf_counter) -- the whole call: the rows' upload, the derivation, the node tables, the kernels, the results' download.
Prints one JSON line: median and spread over --reps calls after one warm-up for both calls and their ratio per grid, and whether
the two calls' total columns agree to the bit."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from base_amd import abi, engine, synth  # noqa: E402


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
    ap.add_argument("--grids", type=int, nargs="+", default=[4, 8], help="K = Q of each grid")
    ap.add_argument("--mass-bins", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    torch = events()
    pack_d = synth.make_pack("parsec", 8)
    truth = synth.default_params(pack_d)
    cl = synth.make_cluster(pack_d, a.stars, seed=9001, truth=truth, wd_frac=a.wd_frac)
    rows = synth.walker_params(truth, a.rows, seed=3, scale=0.3)
    m_up = float(pack_d["m_wd_up"])
    nb = a.mass_bins
    edges = 0.1 * (m_up / 0.1) ** (np.arange(nb + 1) / nb)
    res = dict(stars=a.stars, rows=a.rows, n_filt=8, mass_bins=nb, clock="HIP events and host" if torch is not None else "host")
    key = "event_ms_median" if torch is not None else "host_ms_median"
    for g in a.grids:
        eng = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cl), synth.default_priors(pack_d, truth),
                            abi.make_options(marg_iso_increm=g, marg_n_q=g), device=0)
        n_cells = nb * g
        if n_cells > abi.HIST_MAX_BINS or n_cells > abi.RH_MAX_CELLS:
            raise SystemExit(f"{nb} mass bins x {g} ratios: b9_mass_hist has no call of as many bins")
        hist_edges = 0.1 * (m_up / 0.1) ** (np.arange(n_cells + 1) / n_cells)
        eng.ratio_hist(rows[:2], edges)                        # warm-up: buffers, code object
        eng.mass_hist(rows[:2], hist_edges, abi.HQ_PRIMARY)
        t_ratio, (star, rws) = timed(lambda: eng.ratio_hist(rows, edges), a.reps, torch)
        t_hist, (hstar, hrws) = timed(lambda: eng.mass_hist(rows, hist_edges, abi.HQ_PRIMARY), a.reps, torch)
        cells = rws[:, :-1].reshape(a.rows, nb, g)
        res[f"grid{g}x{g}"] = dict(wd_stage=eng.n_wd_stars(), cells=n_cells, ratio_hist=t_ratio, mass_hist_same_columns=t_hist,
                                   ratio_of_times=t_ratio[key] / t_hist[key], ms_per_row=t_ratio[key] / a.rows,
                                   star_rows_per_s=a.rows * a.stars / (t_ratio[key] * 1e-3),
                                   total_column_same_bits=bool(np.array_equal(star[:, -1], hstar[:, -1]) and np.array_equal(rws[:, -1], hrws[:, -1])),
                                   expected_members=float(rws[:, -1].mean()), expected_members_in_range=float(cells.sum(axis=(1, 2)).mean()),
                                   binary_fraction_all=float((cells[:, :, 1:].sum(axis=(1, 2)) / cells.sum(axis=(1, 2))).mean()))
        eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
