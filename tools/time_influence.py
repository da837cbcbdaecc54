"""Time b9_star_influence against b9_pointwise (the walk both share) and against the route the library had before -- marginalised
b9_logpost with per-star values copied back, reduced in numpy -- on the same catalogue and rows in one process: 20k stars (1000
of them WD-stage) x 256 rows x 8 filters (PARSEC-shaped pack) at the 4 x 4 grid.  Every call is synchronous and bracketed by HIP
events on the null stream (tools/time_pointwise.py's HipEvents) -- the whole call, copies included.  Prints one JSON line:
medians over --reps calls after one warm-up for Q = 1, 5 and 12 with and without the two groups (ms / wd), all with the
--tail-value tail (49: what starInfluence picks for 256 rows); b9_pointwise with the same tail; the old route; the ratios."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from base_amd import abi, engine, synth  # noqa: E402
from time_pointwise import HipEvents, timed  # noqa: E402


def numpy_route(eng, rows, q, group, n_groups):
    """What a caller did before the call existed: every (row, star) value back (b9_logpost in marginalised mode), then the
    weights, their moments and the groups' sums in numpy."""
    _, v = eng.logpost(rows, perstar=True)                               # [rows, stars]
    r = -v
    w = np.exp(r - r.max(axis=0))
    sneg, sneg2 = w.sum(axis=0), (w * w).sum(axis=0)
    wq, wq2 = w.T @ q, w.T @ (q * q)
    cv = (v - v.mean(axis=0)).T @ (q - q.mean(axis=0))
    grp = np.stack([v[:, group == g].sum(axis=1) for g in range(n_groups)], axis=1)
    return sneg, sneg2, wq, wq2, cv, grp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=20000)
    ap.add_argument("--wd-frac", type=float, default=0.05)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--filters", type=int, default=8)
    ap.add_argument("--increm", type=int, default=4)
    ap.add_argument("--ratios", type=int, default=4)
    ap.add_argument("--tail", type=int, default=49)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--once", type=str, default="", help="run one configuration once after the warm-up (for a kernel trace): q<Q>[g], e.g. q5g")
    a = ap.parse_args()
    pack_d = synth.make_pack("parsec", a.filters)
    truth = synth.default_params(pack_d)
    rows = synth.walker_params(truth, a.rows, seed=3, scale=0.3)
    q = np.random.default_rng(5).standard_normal((a.rows, 12))
    cl = synth.make_cluster(pack_d, a.stars, seed=9001, truth=truth, wd_frac=a.wd_frac)
    group = (np.asarray(cl["stage"]) == abi.STAGE_WD).astype(np.int32)
    pack, stars, priors = abi.make_pack(pack_d), abi.make_stars(cl), synth.default_priors(pack_d, truth)
    eng = engine.Engine(pack, stars, priors, abi.make_options(marg_iso_increm=a.increm, marg_n_q=a.ratios), device=0)
    eng.pointwise(rows[:2], a.tail)                                      # warm-up: buffers, code object
    eng.star_influence(rows[:2], q[:2], a.tail, group, 2)
    if a.once:
        Q, g = int(a.once.strip("qg")), a.once.endswith("g")
        eng.star_influence(rows, q[:, :Q], a.tail, group if g else None, 2 if g else 0)
        eng.close()
        return
    ev = HipEvents()
    med = lambda x: float(np.median(x))      # noqa: E731
    out = dict(stars=eng.n_stars, wd_stage=eng.n_wd_stars(), rows=a.rows, n_filt=a.filters, increm=a.increm, ratios=a.ratios, tail_len=a.tail, reps=a.reps)
    _, dev, (pw_acc, _, _) = timed(lambda: eng.pointwise(rows, a.tail, want_rows=False), a.reps, ev)
    out["pointwise_ms"] = pw = med(dev)
    for Q in (1, 5, 12):
        for g in (False, True):
            _, dev, (acc, _, grp) = timed(lambda: eng.star_influence(rows, q[:, :Q], a.tail, group if g else None, 2 if g else 0), a.reps, ev)
            key = f"influence_q{Q}{'_groups' if g else ''}_ms"
            out[key] = med(dev)
            out[key.replace("_ms", "_over_pointwise")] = med(dev) / pw
    out["head_equals_pointwise"] = bool(np.array_equal(acc[:, [abi.INF_RMAX, abi.INF_SNEG]], pw_acc[:, [abi.PW_RMAX, abi.PW_SNEG]]))
    out["finite_group_rows"] = int(np.isfinite(grp).all(axis=1).sum())
    eng.close()
    # the route the library had: a context in marginalised mode on the same grid
    eng = engine.Engine(pack, stars, priors, abi.make_options(mode=abi.MODE_MARGINALISED, marg_iso_increm=a.increm, marg_n_q=a.ratios), device=0)
    numpy_route(eng, rows[:2], q[:2, :5], group, 2)
    _, dev, _ = timed(lambda: eng.logpost(rows, perstar=True), a.reps, ev)
    out["logpost_perstar_ms"] = med(dev)
    wall, _, old = timed(lambda: numpy_route(eng, rows, q[:, :5], group, 2), max(3, a.reps // 4), ev)
    out["logpost_plus_numpy_q5_groups_ms"] = med(wall)
    out["old_route_over_influence_q5_groups"] = med(wall) / out["influence_q5_groups_ms"]
    out["old_route_bytes_back"] = int(8 * a.rows * eng.n_stars)
    out["influence_bytes_back_q5_groups"] = int(8 * (eng.n_stars * (abi.INF_N(5) + a.tail) + a.rows * 2))
    eng.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
