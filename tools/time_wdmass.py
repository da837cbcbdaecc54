"""Time one b9_sample_wd_mass call on the C3 shape: 20k stars x 8 filters (PARSEC-shaped pack), 5 % WD-stage, 256 rows,
512 nodes, with HIP events (torch.cuda.Event) around the synchronous call -- the whole call: the rows' upload, the
derivation, both kernels, the outputs' download.  Prints one JSON line: median and spread over --reps calls after one
warm-up, and (row, star, node) evaluations per second.  With --sample-mass-rows R it also times the only other route to
the same ZAMS draws, b9_sample_mass at marg_iso_increm = n_nodes / 8 on the same catalogue, on the first R rows."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from base_amd import abi, engine, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=20000)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--nodes", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sample-mass-rows", type=int, default=0)
    a = ap.parse_args()
    pack_d = synth.make_pack("parsec", 8)
    truth = synth.default_params(pack_d)
    cl = synth.make_cluster(pack_d, a.stars, seed=9001, truth=truth, wd_frac=0.05)
    rows = synth.walker_params(truth, a.rows, seed=3, scale=0.3)
    eng = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cl), synth.default_priors(pack_d, truth),
                        abi.make_options(marg_iso_increm=max(1, a.nodes // 8), marg_n_q=8), device=0)
    n_wd = eng.n_wd_stars()
    eng.sample_wd_mass(rows, a.nodes, seed=1)                 # warm-up: buffers, code object
    ms = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        g = eng.sample_wd_mass(rows, a.nodes, seed=1)
        ms.append((time.perf_counter() - t0) * 1e3)
    med = float(np.median(ms))
    out = dict(stars=a.stars, wd_stage=n_wd, rows=a.rows, nodes=a.nodes, n_filt=8, call_ms_median=med, call_ms_min=float(min(ms)),
               call_ms_max=float(max(ms)), call_ms=ms, evals_per_s=a.rows * n_wd * a.nodes / (med * 1e-3),
               ms_per_row=med / a.rows, drawn=int(np.sum(g["zams"] > 0)))
    if a.sample_mass_rows > 0:
        r = rows[:a.sample_mass_rows]
        eng.sample_mass(r[:1], seed=1)                       # warm-up
        t = time.perf_counter()
        m = eng.sample_mass(r, seed=1)[0]
        dt = time.perf_counter() - t
        out.update(sample_mass_rows=len(r), sample_mass_ms_per_row=dt * 1e3 / len(r), sample_mass_iso_increm=max(1, a.nodes // 8),
                   same_zams=bool(np.array_equal(m[:, g["star_index"]], g["zams"][:len(r)])) if a.nodes % 8 == 0 else None)
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
