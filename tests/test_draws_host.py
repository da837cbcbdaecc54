"""The random outputs against independently stated distributions, on the CPU: the checkers of tests/stat_check.py run on the
oracle's b9o_sample_mass and on mcmc.HostBlockRunner over the oracle -- the twins the GPU reproduces draw for draw
(tests/test_gpu_draws.py runs the same checkers, seeds and shapes on the kernels) -- and, for every checker, a deliberately
wrong reference that it must reject."""
import functools

import numpy as np
import pytest

import numpy_ref
import oracle
import stat_check as sc
from base_amd import abi, mcmc


def draw(pack_d, cl, priors, n_pops, K, Q, rows, seed, row0):
    opt = abi.make_options(mode=abi.MODE_GIVEN_MASS, n_pops=n_pops, marg_iso_increm=K, marg_n_q=Q)
    return oracle.Oracle(abi.make_pack(pack_d), abi.make_stars(cl), priors, opt).sample_mass(rows, seed=seed, row0=row0)[:4]


def draw_wd(pack_d, cl, priors, rows, n_nodes, seed):
    """The oracle's WD grid has 8 K nodes: b9_sample_wd_mass at n_nodes = 8 K draws what b9o_sample_mass draws."""
    assert n_nodes % 8 == 0
    mass, ratio, member, pop = draw(pack_d, cl, priors, 2, n_nodes // 8, 1, rows, seed, 0)
    assert np.all(ratio == 0)
    return mass, pop


# ---- 1. the draws follow the posterior ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pops,same_y", [(1, False), (2, False), (2, True)])
def test_oracle_draws_follow_the_posterior(n_pops, same_y):
    sc.check_mass_posterior(draw, n_pops, same_y)


def test_oracle_row_numbers_above_32_bits_draw_other_numbers():
    """Rows 2^32 - 2 .. 2^32 + 1: the row's high word is part of the key, so rows 2^32 and 2^32 + 1 must not repeat rows 0 and 1."""
    pack_d, cl, priors, par, tb = sc.mass_problem(1)
    rows = np.repeat(par[None], 4, axis=0)
    hi = draw(pack_d, cl, priors, 1, sc.K_MASS, sc.Q_MASS, rows, sc.SEED_DRAW, 2 ** 32 - 2)
    lo = draw(pack_d, cl, priors, 1, sc.K_MASS, sc.Q_MASS, rows, sc.SEED_DRAW, 0)
    assert not np.array_equal(hi[0], lo[0])
    assert not np.array_equal(hi[0][2:], lo[0][:2])                       # same low word, other high word
    for i in range(8):                                                    # and they are draws from the same grid
        sc.draws_to_index(tb, cl, i, hi[0][:, i], hi[1][:, i], hi[3][:, i])


# ---- 2. independence ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def copies(n_pops):
    return sc.check_copies(draw, n_pops)


@pytest.mark.parametrize("n_pops", [1, 2])
def test_oracle_copies_of_one_star_draw_independently(n_pops):
    copies(n_pops)


def test_oracle_wd_copies_draw_independently():
    sc.check_wd_copies(draw_wd, 64)


# ---- 3. the chain ---------------------------------------------------------------------------------------------------------
N_KEEP_A, N_KEEP_B, WALKERS = 10000, 5000, 8          # the GPU runs the same walkers for at least as many steps


def host_chain(pack_d, cl, priors, opt, start, free, steps, n_burn, n_keep, seed):
    orc = oracle.Oracle(abi.make_pack(pack_d), abi.make_stars(cl), priors, abi.make_options(*opt))
    return sc.run_chain(mcmc.HostBlockRunner(orc.logpost), orc.logpost, start, free, steps, n_burn, n_keep, seed)


@functools.lru_cache(maxsize=None)
def chain_a():
    pack_d, cl, priors, mean, opt = sc.target_a_problem()
    chain, rate = host_chain(pack_d, cl, priors, opt, sc.target_a_start(WALKERS), mcmc.DEFAULT_FREE, sc.A_STEPS, sc.A_BURN, N_KEEP_A, sc.SEED_CHAIN_A)
    print(f"target A, host twin: {N_KEEP_A} steps x {WALKERS} walkers, acceptance {rate:.3f}")
    return chain


@functools.lru_cache(maxsize=None)
def chain_b(k):
    pack_d, cl, priors, truth = sc.target_b_problem()
    m, v = sc.target_b_reference(k)
    chain, rate = host_chain(pack_d, cl, priors, (abi.MODE_GIVEN_MASS, 1, 4, 4), sc.target_b_start(k, WALKERS), (k,), (2.4 * np.sqrt(v),),
                             sc.B_BURN, N_KEEP_B, sc.SEED_CHAIN_B)
    print(f"target B, parameter {k}, host twin: {N_KEEP_B} steps x {WALKERS} walkers, acceptance {rate:.3f}")
    return chain


@pytest.mark.parametrize("marginalised", [False, True])
def test_target_a_likelihood_is_constant(marginalised):
    sc.target_a_is_constant(marginalised, 200 if not marginalised else 60)


def test_host_chain_samples_target_a():
    for name, z in sc.check_target_a("target A, host twin", chain_a()).items():
        assert abs(z) <= sc.Z_MAX, name


@pytest.mark.parametrize("k", [abi.P_MOD, abi.P_LOGAGE])
def test_host_chain_samples_target_b(k):
    zm, zv = sc.moments(f"target B, parameter {k}, host twin", chain_b(k)[:, :, 0], *sc.target_b_reference(k))
    assert abs(zm) <= sc.Z_MAX and abs(zv) <= sc.Z_MAX


# ---- 4. the checkers can fail ---------------------------------------------------------------------------------------------
def mutated_prob(change):
    """The posterior of the copied star from numpy terms that `change` has falsified."""
    pack_d, cl, priors, par, tb = sc.copies_problem(1)
    one = sc.subset(cl, np.zeros(1, int))
    return sc.posterior(change(pack_d, one, par)[0])


def test_goodness_of_fit_rejects_sigma_times_1_1():
    fig, idx, pop, prob = copies(1)

    def change(pack_d, one, par):
        one = dict(one, sigma=np.where(one["sigma"] > 0, one["sigma"] * 1.1, one["sigma"]))
        return numpy_ref.marg_terms(pack_d, one, par, sc.K_MASS, sc.Q_MASS)[0]
    assert sc.gof("mutation: sigma x 1.1", idx, mutated_prob(change)) < sc.P_REJECT


def test_goodness_of_fit_rejects_a_dropped_mass_prior():
    fig, idx, pop, prob = copies(1)

    def change(pack_d, one, par):
        t, m, q = numpy_ref.marg_terms(pack_d, one, par, sc.K_MASS, sc.Q_MASS)
        return t - numpy_ref.log_prior_mass(m, pack_d["m_wd_up"])[None]
    assert sc.gof("mutation: no mass prior", idx, mutated_prob(change)) < sc.P_REJECT


def test_population_count_rejects_lambda_plus_0_05():
    fig, idx, pop, prob = copies(2)
    assert abs(sc.binomial_z("correct lambda", int(np.sum(pop == 0)), pop.size, 0.5)) <= sc.Z_MAX
    assert abs(sc.binomial_z("mutation: lambda + 0.05", int(np.sum(pop == 0)), pop.size, 0.55)) > sc.Z_REJECT
    width = len(prob) // 2
    wrong = np.concatenate([0.55 * prob[:width] / 0.5, 0.45 * prob[width:] / 0.5])
    assert sc.gof("mutation: lambda + 0.05, joint table", idx, wrong) < sc.P_REJECT


def test_coincidence_test_rejects_a_reused_counter():
    fig, idx, pop, prob = copies(1)
    assert sc.coincidence_z("mutation: a copy against itself", idx[:, :-1], idx[:, :-1], prob) > sc.Z_REJECT
    # one reused counter among 130: copy 1 drawing with copy 0's numbers
    aliased = idx.copy(); aliased[:, 1] = aliased[:, 0]
    assert sc.worst_pair_z("mutation: copy 1 repeats copy 0", aliased[:, :-1], aliased[:, 1:], prob) > sc.Z_REJECT


def test_independence_test_rejects_a_node_that_follows_the_population():
    fig, idx, pop, prob = copies(2)
    width = len(prob) // 2
    node = idx % width
    top = int(np.argmax(prob[:width]))
    tied = np.where((pop == 1) & (node == top) & (np.arange(node.size).reshape(node.shape) % 4 == 0), top + 1, node)
    assert sc.independence("mutation: population B avoids a node", pop, tied, width) < sc.P_REJECT


def test_moment_tests_reject_wrong_targets_of_a():
    chain = chain_a()
    ref = sc.target_a_moments()
    wrong = dict(ref)
    wrong[abi.P_ABS] = (sc.A_ABS_MEAN, sc.A_SD[abi.P_ABS] ** 2)                        # the untruncated normal
    wrong[abi.P_FEH] = (ref[abi.P_FEH][0], ref[abi.P_FEH][1] * 1.21)                   # sd x 1.1
    wrong[abi.P_MOD] = (ref[abi.P_MOD][0], ref[abi.P_MOD][1] * 1.21)
    fig = sc.check_target_a("mutation: target A", chain, wrong)
    assert abs(fig["absorption mean"]) > sc.Z_REJECT and abs(fig["absorption var"]) > sc.Z_REJECT
    assert abs(fig["[Fe/H] var"]) > sc.Z_REJECT and abs(fig["modulus var"]) > sc.Z_REJECT
    # a shared Box-Muller pair would show as a correlation: here, modulus mixed into [Fe/H] at 10 %
    mixed = chain.copy(); mixed[:, :, 1] += 0.1 * (chain[:, :, 2] - ref[abi.P_MOD][0])
    assert abs(sc.correlation_z("mutation: correlated components", mixed[:, :, 1], mixed[:, :, 2])) > sc.Z_REJECT


def test_moment_test_rejects_a_shifted_posterior_of_b():
    m, v = sc.target_b_reference(abi.P_MOD)
    zm, _ = sc.moments("mutation: modulus + 0.3 sd", chain_b(abi.P_MOD)[:, :, 0], m + 0.3 * np.sqrt(v), v)
    assert abs(zm) > sc.Z_REJECT
