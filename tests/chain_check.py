"""Checks shared by the GPU sampler tests: a recorded chain against the oracle at the states it visited."""
import numpy as np


def oracle_delta(orc, template_row, free, samples, lps):
    """max relative |delta| between recorded chain log-posteriors and the oracle at the recorded positions; every
    DISTINCT visited state is evaluated once (a rejected step repeats its predecessor's row)."""
    flat = samples.reshape(-1, samples.shape[-1])
    uniq, inverse = np.unique(flat, axis=0, return_inverse=True)
    rows = np.repeat(np.asarray(template_row, dtype=np.float64)[None, :], len(uniq), axis=0)
    rows[:, list(free)] = uniq
    want = orc.logpost(rows)[inverse.ravel()]
    got = lps.reshape(-1)
    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    fin = np.isfinite(want)
    return float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin])))), len(uniq)
