"""The reductions over a saved chain state a star's membership ONCE (base_amd/csrc/b9_chain_walk.hip.h: the node walk, the merge
of the four waves' shares, star_finish; the WD-stage steps), pinned here from outside: the membership column that
b9_star_moments, b9_mass_hist and b9_phot_resid accumulate over the same rows is the same BITS -- p per (row, star) comes out
of the same S0 arithmetic in all three, and each call adds its rows in ascending order with one plain add each.

The catalogue is case 1 of tests/test_gpu_moments.py (dsed, 5 filters, 130 stars, a tenth of them WD-stage), built with one and
with two populations, on a 2 x 2 grid over 33 rows: one more than a chunk of any of the three calls, so a chunk seam is crossed.
b9_mass_hist takes 33 bins -- two tiles of bins, the total column written by the first -- for each of its three quantities.
MS/RGB-stage and WD-stage stars go through different kernels and are asserted separately."""
import numpy as np
import pytest

from base_amd import abi, synth
from conftest import build_problem

pytestmark = pytest.mark.gpu

N_ROWS, N_BINS, K, Q = 33, 33, 2, 2


@pytest.fixture(scope="module", params=[1, 2], ids=["one_population", "two_populations"])
def columns(request):
    """The membership columns of the three calls (mass_hist's per quantity), and the WD-stage mask."""
    from base_amd import engine
    n_pops = request.param
    pack_d, cl, pack, stars, priors, _ = build_problem("dsed", 5, n_stars=130, wd_frac=0.1, n_y=3 if n_pops == 2 else 1, n_pops=n_pops, seed=12)
    rows = synth.walker_params(cl["truth"], N_ROWS, seed=3, scale=0.3, n_pops=n_pops)
    if n_pops == 2:
        rows[:, abi.P_LAMBDA] = np.clip(rows[:, abi.P_LAMBDA], 0.05, 0.95)
    edges = np.linspace(0.05, 2.0 * float(pack_d["m_wd_up"]), N_BINS + 1)
    eng = engine.Engine(pack, stars, priors, abi.make_options(mode=abi.MODE_GIVEN_MASS, n_pops=n_pops, marg_iso_increm=K, marg_n_q=Q))
    try:
        out = {"star_moments": eng.star_moments(rows)[:, abi.MOM_MEMBER].copy(), "phot_resid": eng.phot_resid(rows, want_rows=False)[0][:, 1].copy()}
        for name, q in (("primary", abi.HQ_PRIMARY), ("secondary", abi.HQ_SECONDARY), ("system", abi.HQ_SYSTEM)):
            out["mass_hist " + name] = eng.mass_hist(rows, edges, q, want_rows=False)[0][:, N_BINS].copy()
    finally:
        eng.close()
    wd = np.asarray(cl["stage"]) == abi.STAGE_WD
    assert wd.sum() >= 5 and (~wd).sum() >= 100
    return out, wd


@pytest.mark.parametrize("stage", ["ms_rgb", "wd"])
def test_membership_column_is_the_same_bits(columns, stage):
    out, wd = columns
    sel = wd if stage == "wd" else ~wd
    ref = out["star_moments"][sel]
    assert np.all(ref >= 0) and ref.max() > 1.0                          # members, over many rows: not a column of zeros
    for name, col in out.items():
        differ = np.flatnonzero(col[sel] != ref)
        print(f"{stage}: {name}: {len(differ)} of {sel.sum()} stars differ from star_moments")
        assert np.array_equal(col[sel], ref), name
