"""The bytes of every table file the programs over a saved chain write (docs/FORMATS.md), on the CPU: tests/golden/host_files/
holds what libbase9host's writers made of the fixed tables of tests/golden/make_host_files.py when the fixtures were committed --
before the twelve writers became one column list each over b9h::write_table --, and the library of this tree must write the same
bytes: header words, separators, %.0f / %ld / %.6f / %.17g per column, the optional pPop2 column, -0, 1e300, inf and nan.
.modelCompare comes from modelScore --compareTo (no GPU context); .rowLpd needs a GPU run and is left to test_gpu_pointwise.py."""
import os
import sys

import numpy as np
import pytest

from base_amd import hostlib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_host_files  # noqa: E402


@pytest.fixture(scope="module")
def host():
    from base_amd import host_build
    host_build.build_host()
    return hostlib.load()


def test_every_file_kind_is_written_byte_for_byte(host, tmp_path):
    make_host_files.write_all(str(tmp_path))
    want_dir = os.path.join(GOLDEN, "host_files")
    names = sorted(os.listdir(want_dir))
    assert names == sorted(os.listdir(tmp_path)) and len(names) == 15
    for name in names:
        with open(os.path.join(want_dir, name), "rb") as f, open(tmp_path / name, "rb") as g:
            assert g.read() == f.read(), name


def test_an_unwritable_path_is_an_error(host, tmp_path):
    m = make_host_files
    bad = str(tmp_path / "no_such_directory" / "out")
    writers = [lambda: hostlib.write_star_summary(bad, m.IDS, m.STAR_ACC, 2),               # %.0f and %.6f, labelled
               lambda: hostlib.write_wd_summary(bad, m.IDS, m.WD_ACC, 1),
               lambda: hostlib.write_mass_function(bad, m.MASS_FUNCTION),                    # %.6f, no label column
               lambda: hostlib.write_star_mass_hist(bad, m.IDS, m.STAR_HIST, 400),           # %ld
               lambda: hostlib.write_star_intervals(bad, m.IDS, m.LEVELS, m.STAR_INTERVALS),  # %.17g and %.0f
               lambda: hostlib.write_phot_resid(bad, m.IDS, m.FILTERS, m.PHOT_RESID),        # %.17g, labelled
               lambda: hostlib.write_filter_resid(bad, m.FILTERS, m.FILTER_RESID),
               lambda: hostlib.write_pointwise(bad, m.IDS, m.POINTWISE),
               lambda: hostlib.write_model_score(bad, m.MODEL_SCORE)]                        # one line of named values
    for w in writers:
        with pytest.raises(hostlib.HostError, match="cannot write"):
            w()
    assert not os.path.exists(os.path.dirname(bad))


def test_the_fixtures_read_back(host):
    """What the bytes mean: the readers of hostlib give the tables back (%.17g to the bit, nan where nan was written)."""
    m = make_host_files
    d = os.path.join(GOLDEN, "host_files")
    ids, cols, tab = hostlib.read_pointwise(os.path.join(d, "t.pointwise"))
    assert ids == m.IDS and cols == list(hostlib.POINTWISE_COLUMNS)
    assert np.array_equal(tab, m.POINTWISE, equal_nan=True) and np.signbit(tab[2, 3])
    ids, cols, tab = hostlib.read_star_summary(os.path.join(d, "pops2.starSummary"))
    assert ids == m.IDS and cols == list(hostlib.STAR_TABLE_COLUMNS)
    assert hostlib.read_star_summary(os.path.join(d, "pops1.starSummary"))[1] == list(hostlib.STAR_TABLE_COLUMNS[:7])
    np.testing.assert_allclose(tab[0], hostlib.star_table(m.STAR_ACC)[0], rtol=0, atol=5.0000001e-7)
