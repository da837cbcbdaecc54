"""The comparator of b9_wd_moments against tests/wdmoments_ref.py, and the parity fixtures, shared by the CPU tests
(tests/test_wdmoments_host.py: every mutation of the reference is rejected by it, the fixtures' conditions hold) and the
GPU tests (tests/test_gpu_wdmoments.py)."""
import functools

import numpy as np

import wdmoments_ref as wr
from base_amd import abi, synth
from conftest import build_problem

RTOL = 1e-9               # the project's per-star tolerance; b9_wd_moments prunes nothing, so there is no N e^-40 term
TIE_RTOL = 1e-12          # b9_wd_moments at 8 K nodes against b9_star_moments' columns: another order of summation (test_ties_to_star_moments)
A_MAX = 1e5               # largest weighted amplification of an error in prec (test_gpu_wdmass.py::check_derived's cap)

PER_STAR = ("obs", "sigma", "mass1", "mass_ratio", "clust_prior", "stage", "wd_type", "is_field", "pop")


def subset(cl, sel):
    """The cluster dict reduced to the stars `sel` (mask or index array)."""
    out = dict(cl)
    for k in PER_STAR:
        out[k] = np.ascontiguousarray(np.asarray(cl[k])[sel])
    return out


def wd_problem(name, n_filt, n_stars, n_y=1, n_pops=1, wd_frac=0.25, seed=12, keep=None, **kw):
    """tests/test_gpu_wdmass.py::wd_problem: the WD-stage stars of a synthetic cluster as a catalogue of their own."""
    pack_d, cl, _, _, priors, _ = build_problem(name, n_filt, n_stars=n_stars, wd_frac=wd_frac, n_y=n_y, n_pops=n_pops, seed=seed, **kw)
    idx = np.flatnonzero(np.asarray(cl["stage"]) == abi.STAGE_WD)
    return pack_d, subset(cl, idx if keep is None else idx[:keep]), priors


def rows_for(cl, n_rows, seed, n_pops):
    rows = synth.walker_params(cl["truth"], n_rows, seed=seed, scale=0.3)
    if n_pops == 2:
        rows[:, abi.P_LAMBDA] = np.clip(rows[:, abi.P_LAMBDA], 0.05, 0.95)
    return rows


def opts(n_pops=1, K=1, n_q=1):
    return abi.make_options(mode=abi.MODE_GIVEN_MASS, n_pops=n_pops, marg_iso_increm=K, marg_n_q=n_q)


def assert_close(got, want, floor, what=""):
    """Every column at rtol = 1e-9; the value columns also get atol = 1e-9 p sum w |v| from the reference (`floor`, shaped as
    `want`): a sum of terms of both signs is only good relative to the sum of their magnitudes."""
    got, want, floor = np.asarray(got), np.asarray(want), np.asarray(floor)
    assert got.shape == want.shape, (got.shape, want.shape)
    for c in range(wr.N):
        atol = RTOL * floor[..., c] if c in wr.VALUE_COLS else 1e-300
        bad = ~(np.abs(got[..., c] - want[..., c]) <= atol + RTOL * np.abs(want[..., c]))
        if bad.any():
            k = np.argwhere(bad)[0]
            raise AssertionError(f"{what} column {c}: {int(bad.sum())} of {bad.size} differ; first at {tuple(k)}: "
                                 f"got {got[..., c][tuple(k)]!r}, want {want[..., c][tuple(k)]!r}")


def rejects(check, *args, **kw):
    try:
        check(*args, **kw)
    except AssertionError:
        return True
    return False


# (name, filters, n_y, populations, nodes): test_gpu_wdmass.py's wd_problem on 600 stars -- 150 WD-stage stars -- and 6 rows from
# synth.walker_params(truth, 6, seed=3, scale=0.3)
PARITY = {"parsec": ("parsec", 8, 1, 1, 512), "dsed": ("dsed", 5, 3, 2, 512), "girardi": ("girardi", 3, 1, 1, 64)}


@functools.lru_cache(maxsize=None)
def parity_fixture(key):
    """(pack_d, cl, priors, rows, n_pops, n_nodes, x [6, 150, 16], floor [6, 150, 16], A [6, 150]): computed once and shared;
    nobody changes it."""
    name, n_filt, n_y, n_pops, n_nodes = PARITY[key]
    pack_d, cl, priors = wd_problem(name, n_filt, 600, n_y=n_y, n_pops=n_pops)
    rows = rows_for(cl, 6, 3, n_pops)
    ref = [wr.increments(pack_d, cl, par, n_pops, n_nodes, want_extra=True) for par in rows]
    x, floor, amp = (np.stack([r[k] for r in ref]) for k in range(3))
    for a in (rows, x, floor, amp):
        a.setflags(write=False)
    return pack_d, cl, priors, rows, n_pops, n_nodes, x, floor, amp


@functools.lru_cache(maxsize=None)
def seam_fixture():
    """(pack_d, cl, priors, rows [1], n_nodes): a WD-stage catalogue whose cooled weight lies strictly between 0 and MEMBER.
    Pack A of tests/wd_seams.py has a band of masses above the AGB tip whose precursor is not dead yet (prec >= logAge:
    magnitudes -4.0, no cooling age); at its row 0 and 64 nodes the first 5 nodes lie in it.  The stars are given observations
    between those nodes' magnitudes and a cooled WD's, with errors of 4 mag, so that both kinds of node carry weight."""
    import wd_seams
    pack_d, rows = wd_seams.packs()["A"]
    par = np.array(rows[0], dtype=np.float64)
    cl = synth.make_cluster(pack_d, 200, seed=12, truth=par, wd_frac=0.25, n_pops=1)
    cl = subset(cl, np.flatnonzero(np.asarray(cl["stage"]) == abi.STAGE_WD)[:6])
    obs = np.asarray(cl["obs"], dtype=np.float64)
    alive = -4.0 + par[abi.P_MOD] + (np.asarray(pack_d["abs_coeff"]) - 1.0) * par[abi.P_ABS]
    frac = np.linspace(0.38, 0.5, len(obs))[:, None]
    cl["obs"] = np.ascontiguousarray(alive + frac * (obs - alive))
    cl["sigma"] = np.full_like(np.asarray(cl["sigma"], dtype=np.float64), 4.0)
    return pack_d, cl, synth.default_priors(pack_d, par, 1), par[None, :].copy(), 64


# ---- the statistical check: b9_sample_wd_mass's draws (or numpy's from the reference weights) against a table ---------------
STAT_SEED = 20240607      # checked on the CPU: numpy's draws from the reference weights with this seed pass stat_z's bound
#                           (tests/test_wdmoments_host.py::test_statistical_check_passes_on_numpy_draws_...)
STAT_NODES = 256
STAT_DRAWS = 4000


def stat_problem():
    """test_gpu_wdmass.py::stat_problem: one WD-stage star, one row repeated STAT_DRAWS times."""
    pack_d, cl, priors = wd_problem("parsec", 8, 400, keep=1)
    rows = np.repeat(rows_for(cl, 1, 3, 1), STAT_DRAWS, axis=0)
    return pack_d, cl, priors, rows


def stat_z(pack_d, cl, rows, draws, tab):
    """z of the mean drawn zams (all draws) and of the mean drawn wd_mass and log_cool_age among the draws with
    log_teff != 0, against the table `tab` ([1, 16], hostlib.WD_TABLE_COLUMNS) of the one star; the variances are the
    REFERENCE's.  A quantity whose skewness fails moments_ref.SKEW_GUARD is left out; one to which the table gives no spread
    while the reference does is z = inf."""
    import moments_ref
    mo_m, mo_wd, mo_cool, _ = wr.star_moments(wr.star_nodes(pack_d, cl, rows[0], 1, STAT_NODES)[0])
    cooled = np.asarray(draws["log_teff"])[:, 0] != 0 if np.asarray(draws["log_teff"]).ndim == 2 else np.asarray(draws["log_teff"]) != 0
    col = lambda k: np.asarray(draws[k]).reshape(len(cooled))            # noqa: E731
    z = []
    for mo, x, mean_col in ((mo_m, col("zams"), 3), (mo_wd, col("wd_mass")[cooled], 5), (mo_cool, col("log_cool_age")[cooled], 9)):
        n = len(x)
        if mo is None or n == 0 or not mo[1] > 0 or abs(mo[2]) / np.sqrt(n) > moments_ref.SKEW_GUARD:
            continue
        z.append(np.inf if not tab[0, mean_col + 1] > 0 else (x.mean() - tab[0, mean_col]) / np.sqrt(mo[1] / n))
    return np.array(z)


def reference(pack_d, cl, rows, n_pops, n_nodes):
    """(x [rows, n_wd, 16], floor) of the reference, row by row."""
    ref = [wr.increments(pack_d, cl, par, n_pops, n_nodes, want_extra=True) for par in np.asarray(rows).reshape(-1, abi.B9_NPARAM)]
    return np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])


def assert_accumulated(got, x, floor, what=""):
    """An accumulator against the reference's rows added in ascending order (the floors add up)."""
    want = np.zeros(x.shape[1:])
    for r in range(x.shape[0]):
        want = want + x[r]
    assert_close(got, want, floor.sum(axis=0), what)
