"""The random outputs of the kernels against independently stated distributions: b9_sample_mass and b9_sample_wd_mass against
the numpy posterior over the grid (goodness of fit, membership, population counts, independence between stars, rows and
populations), and the device Metropolis block (k_mcmc_step, k_mcmc_tree, k_marg_step) against analytic targets and a
brute-force one-dimensional posterior.  Checkers, problems, seeds: tests/stat_check.py; the CPU twins of these tests
(tests/test_draws_host.py) run the same on the oracle and the host twin."""
import numpy as np
import pytest

import oracle
import stat_check as sc
from base_amd import abi, mcmc

pytestmark = pytest.mark.gpu


def draw(pack_d, cl, priors, n_pops, K, Q, rows, seed, row0):
    from base_amd import engine
    opt = abi.make_options(mode=abi.MODE_GIVEN_MASS, n_pops=n_pops, marg_iso_increm=K, marg_n_q=Q)
    eng = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cl), priors, opt)
    try:
        return eng.sample_mass(rows, seed=seed, row0=row0)
    finally:
        eng.close()


def draw_wd(pack_d, cl, priors, rows, n_nodes, seed):
    from base_amd import engine
    eng = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cl), priors, abi.make_options(mode=abi.MODE_GIVEN_MASS, n_pops=2, marg_iso_increm=1, marg_n_q=1))
    try:
        g = eng.sample_wd_mass(rows, n_nodes, seed=seed, row0=0)
    finally:
        eng.close()
    assert g["zams"].shape == (len(rows), sc.N_COPIES)
    return g["zams"], g["pop"]


# ---- 1. b9_sample_mass follows the posterior --------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pops,same_y", [(1, False), (2, False), (2, True)])
def test_draws_follow_the_posterior(n_pops, same_y):
    sc.check_mass_posterior(draw, n_pops, same_y)


def test_row_numbers_above_32_bits():
    """Four rows at row0 = 2^32 - 2 (the row's high word goes into the key): the oracle's draws node for node where the
    oracle's margin allows, and other draws than rows 0 .. 3 -- rows 2^32, 2^32 + 1 in particular do not repeat rows 0, 1."""
    pack_d, cl, priors, par, tb = sc.mass_problem(1)
    rows = np.repeat(par[None], 4, axis=0)
    hi = draw(pack_d, cl, priors, 1, sc.K_MASS, sc.Q_MASS, rows, sc.SEED_DRAW, 2 ** 32 - 2)
    lo = draw(pack_d, cl, priors, 1, sc.K_MASS, sc.Q_MASS, rows, sc.SEED_DRAW, 0)
    opt = abi.make_options(mode=abi.MODE_GIVEN_MASS, n_pops=1, marg_iso_increm=sc.K_MASS, marg_n_q=sc.Q_MASS)
    om, oq, omem, opop, margin = oracle.Oracle(abi.make_pack(pack_d), abi.make_stars(cl), priors, opt).sample_mass(rows, seed=sc.SEED_DRAW, row0=2 ** 32 - 2)
    safe = margin > 1e-6
    assert safe.sum() >= 28
    np.testing.assert_allclose(hi[0][safe], om[safe], rtol=1e-12, atol=0)
    assert np.array_equal(hi[1][safe], oq[safe])
    assert not np.array_equal(hi[0], lo[0])
    assert not np.array_equal(hi[0][2:], lo[0][:2])


# ---- 2. independence ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pops", [1, 2])
def test_copies_of_one_star_draw_independently(n_pops):
    sc.check_copies(draw, n_pops)


def test_wd_sampler_copies_draw_independently():
    sc.check_wd_copies(draw_wd, 65)


# ---- 3. the device chain samples the posterior --------------------------------------------------------------------------------
def device_chain(monkeypatch, env, pack_d, cl, priors, opt, depth, start, free, steps, n_burn, n_keep, seed):
    from base_amd import engine
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = engine.Engine(abi.make_pack(pack_d), abi.make_stars(cl), priors, abi.make_options(*opt))
    try:
        if depth:
            assert eng.step_depth(len(start)) == depth
        return sc.run_chain(mcmc.DeviceBlockRunner(eng), eng.logpost, start, free, steps, n_burn, n_keep, seed)
    finally:
        eng.close()


@pytest.mark.parametrize("form,env,marginalised,depth,walkers,n_keep", [
    ("k_mcmc_step", {"B9_TREE_DEPTH": "1"}, False, 1, 8, 20000),
    ("k_mcmc_tree", {"B9_TREE_DEPTH": "3"}, False, 3, 1, 160000),
    ("k_marg_step", {}, True, 0, 2, 80000),
])
def test_device_chain_samples_target_a(monkeypatch, form, env, marginalised, depth, walkers, n_keep):
    sc.target_a_is_constant(marginalised, 200 if not marginalised else 60)
    pack_d, cl, priors, mean, opt = sc.target_a_problem(marginalised)
    chain, rate = device_chain(monkeypatch, env, pack_d, cl, priors, opt, depth, sc.target_a_start(walkers), mcmc.DEFAULT_FREE, sc.A_STEPS,
                               sc.A_BURN, n_keep, sc.SEED_CHAIN_A)
    print(f"target A, {form}: {n_keep} steps x {walkers} walkers, acceptance {rate:.3f}")
    for name, z in sc.check_target_a(f"target A, {form}", chain).items():
        assert abs(z) <= sc.Z_MAX, name


@pytest.mark.parametrize("k", [abi.P_MOD, abi.P_LOGAGE])
def test_device_chain_samples_target_b(monkeypatch, k):
    pack_d, cl, priors, truth = sc.target_b_problem()
    m, v = sc.target_b_reference(k)
    chain, rate = device_chain(monkeypatch, {}, pack_d, cl, priors, (abi.MODE_GIVEN_MASS, 1, 4, 4), 0, sc.target_b_start(k, 8), (k,),
                               (2.4 * np.sqrt(v),), sc.B_BURN, 10000, sc.SEED_CHAIN_B)
    print(f"target B, parameter {k}: 10000 steps x 8 walkers, acceptance {rate:.3f}")
    zm, zv = sc.moments(f"target B, parameter {k}", chain[:, :, 0], m, v)
    assert abs(zm) <= sc.Z_MAX and abs(zv) <= sc.Z_MAX
