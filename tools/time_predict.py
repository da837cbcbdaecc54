"""Time one b9_predict_mags call: 1e6 systems, 8 filters (PARSEC-shaped pack), 5 % WD primaries, 30 % binaries, with HIP
events (torch.cuda.Event) around the synchronous call -- the whole call: the derivation, the host <-> device copies of the
systems and their magnitudes, the kernel.  Prints one JSON line (median over --reps calls after one warm-up)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from base_amd import abi, engine, hostlib, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    pack_d = synth.make_pack("parsec", 8)
    row = synth.default_params(pack_d)
    eng = engine.Engine(abi.make_pack(pack_d), device=0)
    tip = eng.derive_isochrone(row)[3]
    m1, q, wt, _ = hostlib.sim_draw_systems(1, 0, a.n, [tip], min_mass=0.15, max_mass=tip, percent_binary=30.0, percent_db=20.0)
    wd = np.random.default_rng(1).random(a.n) < 0.05
    m1[wd] = np.random.default_rng(2).uniform(tip * 1.01, 7.9, int(wd.sum()))
    q[wd] = 0.0
    eng.predict_mags(row, m1, q, wt)                         # warm-up: buffers, code object
    ms = []
    for _ in range(a.reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        mags, stage = eng.predict_mags(row, m1, q, wt)
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    print(json.dumps(dict(n=a.n, n_filt=8, wd_fraction=float(wd.mean()), call_ms_median=float(np.median(ms)), call_ms=ms,
                          wd_stage=int(np.sum(stage == abi.STAGE_WD)))))
    eng.close()


if __name__ == "__main__":
    main()
