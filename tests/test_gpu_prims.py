"""The device primitives every kernel shares -- log_ge1 / log_pos, exp_fast, log1pexp, logaddexp, fdiv and find_bracket's
quotient, the bracket searches, the wave reductions and moves, Philox and u01, the field-star product accumulator, the online
log-sum-exp and the box pruning -- one by one on the GPU, each against a plain high-precision reference and the bound its own
comment states.  The probe library (tests/probes/b9_prims_probe.hip) compiles the shipped headers unchanged under the
library's own flags; the checks are tests/prims_check.py's, which tests/test_prims_host.py shows to reject a mutated subject.
Every test prints the figures it measured (docs/LABNOTES.md section 13 holds them)."""
import pytest

import prims_check as pc
import prims_probe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    return prims_probe.load()


def show(fig):
    for k, v in fig.items():
        print(f"  {k}: {v}")


def test_log_ge1_and_log_pos_within_one_ulp(P):
    show(pc.check_log(P))


def test_exp_fast_within_one_ulp_and_its_edges(P):
    show(pc.check_exp(P))


def test_log1pexp_absolute_accuracy(P):
    """x <= 0: 4e-16 absolute; 0 < x <= 700: 2 ulp.  Beyond 709.78 the result is NaN (recorded): no call site reaches it --
    the flux combines pass (-0.4 ln 10)(s - p) with |s - p| <= 104 mag, logaddexp passes lo - hi <= 0."""
    show(pc.check_log1pexp(P))


def test_logaddexp_against_the_log_sum_exp(P):
    show(pc.check_logaddexp(P))


def test_fdiv_and_find_bracket_quotient_within_one_ulp(P):
    """Finding recorded by the check: whether num == den gives exactly 1 (printed; docs/LABNOTES.md section 13)."""
    show(pc.check_fdiv(P))


def test_bracket_searches_equal_searchsorted(P):
    show(pc.check_searches(P))


def test_lane_down_moves_the_specified_lanes(P):
    pc.check_lane_down(P)


def test_wave_sum_is_the_stated_tree(P):
    show(pc.check_wave_sum(P))


def test_wave_sum7_equals_seven_wave_sums(P):
    pc.check_wave_sum7(P)


def test_wave_max_all_and_broadcasts(P):
    pc.check_wave_max_bcast(P)


def test_philox_known_answers_and_u01_on_the_device(P):
    pc.check_rng(P)


def test_mix_accumulator_against_the_sum_of_logs(P):
    show(pc.check_mix(P))


def test_mix_accumulator_subnormal_factors_recorded(P):
    """A = 1e-310 and 5e-324 with l = -inf: recorded, not asserted -- outside mix_add's stated domain (A is 0 or a normal double):
    b9_load_stars rejects a catalogue whose (1 - p) / prod(filter ranges) is subnormal."""
    for a, (got, err, bound) in pc.mix_subnormal_record(P).items():
        print(f"  A = {a!r}: mix total {got!r}, error {err:.3e}, the normal-range bound {bound:.3e}")


def test_online_log_sum_exp_and_its_merge(P):
    show(pc.check_lse(P))


@pytest.mark.parametrize("nfp", [2, 4, 8, 16])
def test_box_pruning_is_a_rigorous_bound(P, nfp):
    show(pc.check_box(P, nfp))
