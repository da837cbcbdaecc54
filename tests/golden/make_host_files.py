#!/usr/bin/env python3
"""Generates tests/golden/host_files/* -- every kind of table file the programs over a saved chain write, from small fixed
hand-made tables, through libbase9host's own writers (hostlib.write_*) and, for .modelCompare, through modelScore --compareTo
(which needs no GPU).  3 stars, 3 bins, 2 filters, 2 levels; one and two populations where the writer takes the count.  The tables
hold 0, -0.0, a value that needs all 17 digits, 1e300 and -- where the format is %.17g -- inf, -inf and nan; one id is not
alphanumeric.  tests/test_host_files.py regenerates the files and compares them byte for byte: the fixtures pin the writers'
output as it was when they were first committed.  (.rowLpd is written by a modelScore run on a GPU only: test_gpu_pointwise.py.)

    python tests/golden/make_host_files.py        # rewrites the fixtures
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from base_amd import host_build, hostlib  # noqa: E402

IDS = ["s1", "NGC188_12+3.5/b#", "3"]
FILTERS = ["U", "F606W"]
LEVELS = [0.16, 0.5]
D17 = 0.1 + 0.2                        # 0.30000000000000004
INF, NAN = float("inf"), float("nan")

STAR_ACC = np.array([[400, 200.5, 250.5, 330.25, 100.25, 60.5, 50, 20],
                     [0, 0, 0, 0, 0, 0, 0, 0],
                     [3, 1, -0.0, 0.0, 1e300, 0, D17, 1]], dtype=np.float64)
WD_ACC = np.array([[400, 300.5, 200.25] + [1.5 * k + D17 for k in range(12)] + [100.125],
                   [0] * 16,
                   [3, 1, 1, -0.0, 0.0, 1e300, 0, D17, 1, 2, 5, 3, 10, 4, 17, 0.5]], dtype=np.float64)
MASS_FUNCTION = np.array([[0.1, 0.5, 12.25, 1.5, 10.0, 12.0, 14.5, 17.526],
                          [0.5, 2.0, 0.0, -0.0, D17, 1e300, 0, 0],
                          [2.0, 8.0, 3.0000005, 2.9999995, 1e-7, 5e-7, -5e-7, 1]], dtype=np.float64)
STAR_HIST = np.array([[100.0, 250.5, 49.5, 400.0], [0, 0, 0, 0], [D17, -0.0, 1e300, 1e300]], dtype=np.float64)
STAR_INTERVALS = np.array([[0.95, 0.8, 0.75, 0.85, 1.0, 0.95, 1.05, 3, 0],
                           [0.0, NAN, NAN, NAN, NAN, NAN, NAN, 1, 1],
                           [D17, -0.0, -INF, 0.5, 1e300, 7.5, INF, 12, 2]], dtype=np.float64)
PHOT_RESID = np.array([[400, 0.95, 15.25, 0.03, -0.01, 1.1, 14.5, 0.02, 0.005, 0.9],
                       [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                       [3, D17, -0.0, 1e300, INF, -INF, NAN, 0, 1e-300, -1e300]], dtype=np.float64)
FILTER_RESID = np.array([[400] + [0.25 * k - 1 for k in range(15)],
                         [0, -0.0, D17, 1e300, INF, -INF, NAN] + [0] * 9], dtype=np.float64)
POINTWISE = np.array([[400, 0, -3.25, 0.5, -3.75, -3.5, 0.125, -3.625, 0.375],
                      [400, 2, -INF, D17, -INF, -INF, INF, -INF, INF],
                      [0, 0, 0, -0.0, 0, 0, NAN, 1e300, 0]], dtype=np.float64)
POINTWISE_OTHER = np.array([[400, 0, -3.5, 0.5, -4.0, -3.75, 0.25, -4.125, 0.625],
                            [400, 0, -5.0, 1.0, -6.0, -5.5, NAN, -5.5 - D17, 0.5],
                            [10, 0, -1.0, 0.25, -1.25, -1.2, 0.3, -1.125, 0.125]], dtype=np.float64)
MODEL_SCORE = np.array([3, -8.25, D17, -9.75, 1e300, -INF, NAN, 1.5, INF, 1, 0, -0.0], dtype=np.float64)


def write_all(out_dir: str) -> None:
    """Every fixture into out_dir (which exists)."""
    p = lambda name: os.path.join(out_dir, name)     # noqa: E731
    for n_pops in (1, 2):
        hostlib.write_star_summary(p(f"pops{n_pops}.starSummary"), IDS, STAR_ACC, n_pops)
        hostlib.write_wd_summary(p(f"pops{n_pops}.wdSummary"), IDS, WD_ACC, n_pops)
    hostlib.write_mass_function(p("t.massFunction"), MASS_FUNCTION)
    hostlib.write_star_mass_hist(p("t.starMassHist"), IDS, STAR_HIST, 400)
    hostlib.write_star_mass_hist(p("rows0.starMassHist"), IDS, STAR_HIST, 0)
    hostlib.write_star_intervals(p("t.starIntervals"), IDS, LEVELS, STAR_INTERVALS)
    hostlib.write_phot_resid(p("t.photResid"), IDS, FILTERS, PHOT_RESID)
    hostlib.write_filter_resid(p("t.filterResid"), FILTERS, FILTER_RESID)
    hostlib.write_pointwise(p("t.pointwise"), IDS, POINTWISE)
    hostlib.write_pointwise(p("other.pointwise"), IDS, POINTWISE_OTHER)
    hostlib.write_model_score(p("t.modelScore"), MODEL_SCORE)
    # .modelCompare has no C export: modelScore --compareTo reads the two .pointwise files above, before any GPU context exists
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    for base, other in (("t", "other"), ("other", "t")):
        r = subprocess.run([os.path.join(host_build.BIN, "modelScore"), "--outputFileBase", p(base), "--compareTo", p(other)],
                           capture_output=True, text=True, timeout=120, env=env)
        if r.returncode != 0:
            raise RuntimeError("modelScore --compareTo failed: " + r.stderr)


if __name__ == "__main__":
    out = os.path.join(HERE, "host_files")
    os.makedirs(out, exist_ok=True)
    write_all(out)
    print(sorted(os.listdir(out)))
