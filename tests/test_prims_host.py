"""The checks of the device primitives (tests/prims_check.py) on the CPU: they pass on an emulation of each primitive
(tests/probes/b9_prims_emul.cpp, built here with g++ -ffp-contract=off) and REJECT every one of its mutants -- so each check
is shown to have the power to see the error it is there for, without a GPU.  tests/test_gpu_prims.py runs the same checks on
the shipped headers."""
import ctypes
import os
import subprocess

import pytest

import prims_check as pc
from prims_probe import Prims

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MUTANTS = dict(log_coefficient=1, log_ln2_lo_dropped=2, exp_coefficient=3, exp_ln2_lo_dropped=4, bracket_off_by_one_at_len_8=5,
               tree_16_before_32=6, box_without_inv=7, slack_1000_times_smaller=8, f32_below_to_nearest=9)


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("prims") / "libb9prims_emul.so")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-shared", "-fPIC", "-o", so,
           os.path.join(ROOT, "tests", "probes", "b9_prims_emul.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-3000:]
    p = Prims(so)
    p.lib.b9p_set_mutant(ctypes.c_int(0))
    yield p
    p.lib.b9p_set_mutant(ctypes.c_int(0))


SMALL = [2, 3, 7, 8, 9, 10, 16, 17, 33, 64, 65, 73, 80, 129, 513]      # (the GPU test walks every length; 9 is where len == 8)

CHECKS = dict(log=pc.check_log, exp=pc.check_exp, log1pexp=pc.check_log1pexp, logaddexp=pc.check_logaddexp, fdiv=pc.check_fdiv,
              searches=lambda p: pc.check_searches(p, SMALL), lane_down=pc.check_lane_down, wave_sum=pc.check_wave_sum,
              wave_sum7=pc.check_wave_sum7, wave_max_bcast=pc.check_wave_max_bcast, rng=pc.check_rng,
              mix=lambda p: pc.check_mix(p, ks=(1, 7)), lse=pc.check_lse,
              box4=lambda p: pc.check_box(p, 4), box8=lambda p: pc.check_box(p, 8))


@pytest.mark.parametrize("name", list(CHECKS))
def test_checker_passes_on_the_emulation(emul, name):
    emul.lib.b9p_set_mutant(ctypes.c_int(0))
    print(CHECKS[name](emul))


# which checks must reject which mutant
REJECTS = dict(log_coefficient=["log"], log_ln2_lo_dropped=["log"], exp_coefficient=["exp"], exp_ln2_lo_dropped=["exp"],
               bracket_off_by_one_at_len_8=["searches"], tree_16_before_32=["wave_sum", "wave_sum7"],
               box_without_inv=["box4", "box8"], slack_1000_times_smaller=["box4", "box8"], f32_below_to_nearest=["box4", "box8"])


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_checker_rejects_the_mutant(emul, mutant):
    try:
        for name in REJECTS[mutant]:
            emul.lib.b9p_set_mutant(ctypes.c_int(MUTANTS[mutant]))
            with pytest.raises(AssertionError):
                CHECKS[name](emul)
    finally:
        emul.lib.b9p_set_mutant(ctypes.c_int(0))


def test_subnormal_mix_record_runs(emul):
    rec = pc.mix_subnormal_record(emul)
    assert set(rec) == {1e-310, 5e-324}
