"""Bit-for-bit comparison of two builds of libbase9hip.so: sampler chains (tree depths 3 / 2 and the one-step launch, one and two
populations, WD stars) and marginalised per-star values of the shipped library against the variant library named on the command
line -- used when a change must not move a single bit (e.g. the cross-lane sums on DPP / permlane moves, a host-side refactor) --
and the four reductions over a saved chain (b9_star_moments, b9_mass_hist per quantity, b9_phot_resid, b9_pointwise): every
output's bytes -- accumulators, row sums, tail -- of one call over 33 rows and of the same rows split over a continued call, on
3000-star cuts of C3 (WD stars) and C4s (two populations) at 8 filters and of C3 at 16, 33 bins, tail_len 5; and the three calls
on a WD mass grid (b9_sample_wd_mass: all eight outputs; b9_wd_moments; b9_wd_bins: all six quantities at 7 bins on edges from
hostlib.wd_first_ranges) on the same three cuts, 33 rows, 200 nodes (four tiles, the last of 8 nodes), as one call and continued.
    python tools/build_variant.py oldsum   (on the tree to compare against);   python tools/compare_bits.py build/variants/lib_oldsum.so [sampler|chain|wd]   (GPU box)"""
import os, sys, subprocess, pickle
sys.path.insert(0, os.getcwd())
CUT = 3000


def cut(cl, ns):
    return {k: (v[:CUT] if hasattr(v, "__len__") and len(v) == ns else v) for k, v in cl.items()}


def sampler_cases(out):
    import numpy as np
    from base_amd import abi, engine, mcmc, synth
    for name, (pk, nf, ns, wd, ny, npops, W) in {"C1": ("dsed", 8, 10000, 0.0, 1, 1, 1), "C2s": ("parsec", 8, 20000, 0.0, 1, 1, 8), "C3": ("parsec", 8, 20000, 0.05, 1, 1, 1), "C4s": ("parsec", 8, 9000, 0.02, 3, 2, 8), "W2": ("parsec", 5, 30000, 0.01, 1, 1, 2)}.items():
        pack_d = synth.make_pack(pk, nf, n_y=ny); truth = synth.default_params(pack_d)
        cl = synth.make_cluster(pack_d, ns, seed=11, truth=truth, wd_frac=wd, n_pops=npops)
        eng = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cl), synth.default_priors(pack_d, truth, npops), abi.make_options(n_pops=npops))
        free = np.array(mcmc.DEFAULT_FREE if npops == 1 else mcmc.DEFAULT_FREE + (abi.P_Y, abi.P_Y2, abi.P_LAMBDA), dtype=np.int32)
        start = synth.walker_params(truth, W, seed=7, n_pops=npops, scale=0.02); lp = eng.logpost(start)
        chol = np.diag([mcmc.DEFAULT_STEP[int(k)] for k in free]) * 0.3
        r = eng.mcmc_run_block(start, lp, np.arange(W, dtype=np.int32), free, chol, 7, 0, 60)
        out[name] = (lp.tobytes(), r[0].tobytes(), r[1].tobytes(), r[2].tobytes(), r[3].tobytes(), r[4], eng.step_depth(W))
        # marginalised logpost too
        engm = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cut(cl, ns)), synth.default_priors(pack_d, truth, npops), abi.make_options(abi.MODE_MARGINALISED, npops, 4, 4))
        out[name + "m"] = engm.logpost(start, perstar=True)[1].tobytes()


def chain_cases(out):
    import numpy as np
    from base_amd import abi, engine, synth
    R, BINS, TAIL, SPLIT = 33, 33, 5, 13
    # every array's bytes, then a note that the comparison is not one of zeros: the first array's non-zero words
    b = lambda *arrays: tuple(None if a is None else a.tobytes() for a in arrays) + (f"({np.count_nonzero(arrays[0])} of {arrays[0].size} words non-zero)",)      # noqa: E731
    for name, (pk, nf, ns, wd, ny, npops) in {"C3 chain": ("parsec", 8, 20000, 0.05, 1, 1), "C4s chain": ("parsec", 8, 9000, 0.02, 3, 2),
                                              "C3 chain 16f": ("parsec", 16, 20000, 0.05, 1, 1)}.items():
        pack_d = synth.make_pack(pk, nf, n_y=ny); truth = synth.default_params(pack_d)
        cl = cut(synth.make_cluster(pack_d, ns, seed=11, truth=truth, wd_frac=wd, n_pops=npops), ns)
        rows = synth.walker_params(truth, R, seed=7, n_pops=npops, scale=0.1)
        rows[R // 2, abi.P_LOGAGE] = pack_d["log_age"][-1] + 1.0            # one row outside the grid
        edges = np.linspace(0.05, 2.0 * float(pack_d["m_wd_up"]), BINS + 1)
        eng = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cl), synth.default_priors(pack_d, truth, npops), abi.make_options(abi.MODE_GIVEN_MASS, npops, 4, 4))
        a, z = rows[:SPLIT], rows[SPLIT:]
        out[name + " moments"] = b(eng.star_moments(rows), eng.star_moments(z, eng.star_moments(a)))
        for q in (abi.HQ_PRIMARY, abi.HQ_SECONDARY, abi.HQ_SYSTEM):
            sh, rh = eng.mass_hist(rows, edges, q)
            out[name + f" hist q{q}"] = b(sh, rh, eng.mass_hist(z, edges, q, eng.mass_hist(a, edges, q)[0])[0])
        sr, rr = eng.phot_resid(rows)
        out[name + " resid"] = b(sr, rr, eng.phot_resid(z, eng.phot_resid(a)[0])[0])
        acc, tail, lpd = eng.pointwise(rows, TAIL)
        a1 = eng.pointwise(a, TAIL)
        a2 = eng.pointwise(z, TAIL, a1[0], a1[1])
        out[name + " pointwise"] = b(acc, tail, lpd, a2[0], a2[1], a2[2])
        eng.close()


def wd_cases(out):
    import numpy as np
    from base_amd import abi, engine, hostlib, synth
    R, NODES, BINS, SPLIT = 33, 200, 7, 13
    # every array's bytes, then every array's non-zero words (the drawn populations of a one-population case are all zeros)
    b = lambda *arrays: tuple(a.tobytes() for a in arrays) + (" ".join(f"({np.count_nonzero(a)} of {a.size})" for a in arrays) + " words non-zero",)      # noqa: E731
    for name, (pk, nf, ns, wd, ny, npops) in {"C3 wd": ("parsec", 8, 20000, 0.05, 1, 1), "C4s wd": ("parsec", 8, 9000, 0.02, 3, 2),
                                              "C3 wd 16f": ("parsec", 16, 20000, 0.05, 1, 1)}.items():
        pack_d = synth.make_pack(pk, nf, n_y=ny); truth = synth.default_params(pack_d)
        cl = cut(synth.make_cluster(pack_d, ns, seed=11, truth=truth, wd_frac=wd, n_pops=npops), ns)
        rows = synth.walker_params(truth, R, seed=7, n_pops=npops, scale=0.1)
        rows[R // 2, abi.P_LOGAGE] = pack_d["log_age"][-1] + 1.0            # one row outside the grid
        eng = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cl), synth.default_priors(pack_d, truth, npops), abi.make_options(abi.MODE_GIVEN_MASS, npops, 4, 4))
        a, z = rows[:SPLIT], rows[SPLIT:]
        d = eng.sample_wd_mass(rows, NODES, seed=5, row0=3)
        out[name + " sample"] = b(*(d[k] for k in ("zams",) + eng.WD_DERIVED + ("member", "pop")))
        acc = eng.wd_moments(rows, NODES)[0]
        out[name + " moments"] = b(acc, eng.wd_moments(z, NODES, eng.wd_moments(a, NODES)[0])[0])
        lo, hi = hostlib.wd_first_ranges(acc)
        edges = lo[..., None] + (hi - lo)[..., None] * np.linspace(0.0, 1.0, BINS + 1)
        out[name + " bins"] = b(eng.wd_bins(rows, NODES, edges)[0], eng.wd_bins(z, NODES, edges, acc=eng.wd_bins(a, NODES, edges)[0])[0])
        eng.close()


if len(sys.argv) == 4 and sys.argv[1] == "--dump":      # child: run the cases with the library B9_HIP_LIB selects, pickle the bytes
    out = {}
    print("library:", os.environ.get("B9_HIP_LIB", "the tree's own"), file=sys.stderr)
    if sys.argv[3] in ("all", "sampler"): sampler_cases(out)
    if sys.argv[3] in ("all", "chain"): chain_cases(out)
    if sys.argv[3] in ("all", "wd"): wd_cases(out)
    pickle.dump(out, open(sys.argv[2], "wb"))
else:
    if len(sys.argv) not in (2, 3) or not os.path.exists(sys.argv[1]) or (len(sys.argv) == 3 and sys.argv[2] not in ("sampler", "chain", "wd")):
        raise SystemExit("usage: python tools/compare_bits.py <variant libbase9hip.so> [sampler|chain|wd]")
    which = sys.argv[2] if len(sys.argv) == 3 else "all"
    env = dict(os.environ)
    env.pop("B9_HIP_LIB", None)
    subprocess.check_call([sys.executable, __file__, "--dump", "/tmp/new.pkl", which], env=env)
    env["B9_HIP_LIB"] = sys.argv[1]
    subprocess.check_call([sys.executable, __file__, "--dump", "/tmp/old.pkl", which], env=env)
    a, b = pickle.load(open("/tmp/new.pkl", "rb")), pickle.load(open("/tmp/old.pkl", "rb"))
    for k in a:
        print(k, "identical" if a[k] == b[k] else "DIFFERENT", a[k][-1] if not k.endswith("m") else "")
