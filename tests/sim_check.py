"""Helpers shared by the b9_predict_mags tests: the oracle's isochrones at a row, the numpy forward model per population,
and a set of systems that reaches every branch of the forward model."""
import numpy as np

import oracle
from base_amd import synth


def isochrone_tips(pack, row, n_pops):
    """The oracle's (first EEP, mass, mags, AGB tip) at `row` for each population."""
    lib = oracle.load()
    return [oracle.derive_isochrone(lib, pack, row, k) for k in range(n_pops)]


def forward_by_pop(pack_d, row, m1, q, wt, pop):
    """synth.forward_mags of every system at `row`, each in its own population."""
    out = np.empty((len(m1), pack_d["n_filt"]))
    for k in (0, 1):
        s = pop == k
        if s.any():
            out[s] = synth.forward_mags(pack_d, row, m1[s], q[s], wt[s], pop=k)
    return out


def branch_systems(isos, m_wd_up, n_pops, rng):
    """Every branch: below the first mass, MS/RGB singles and binaries, WD DA / DB, above m_wd_up, a NS with a companion."""
    m1, q, wt, pop = [], [], [], []
    for k in range(n_pops):
        _, mass, _, tip = isos[k]
        ms = rng.uniform(mass[0], tip, 60)
        cases = [(mass[0] * 0.7, 0.0), (mass[0] * 0.9, 0.5)] + [(m, 0.0) for m in ms[:30]] + \
                [(m, rng.uniform(0.05, 1.0)) for m in ms[30:]] + [(m, 0.0) for m in rng.uniform(tip * 1.01, m_wd_up * 0.99, 20)] + \
                [(m_wd_up * 1.2, 0.0), (m_wd_up * 1.1, 0.2), (tip, 0.0), (mass[0], 0.0)]
        for a, b in cases:
            m1.append(a); q.append(b); wt.append(int(rng.random() < 0.5)); pop.append(k)
    return np.array(m1), np.array(q), np.array(wt, np.int32), np.array(pop, np.int32)
