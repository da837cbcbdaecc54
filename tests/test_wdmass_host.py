"""b9_sample_wd_mass without a GPU: the numpy helper tests/wd_check.py against the forward model the GPU is already tested
against, the new ABI symbols in the header / the library / the Python binding, and the new kernels' instances and scratch
in the cross-compiled gfx950 code, and the .res reader sampleMass and sampleWDMass share."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import wd_check
from base_amd import abi, hostlib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n_carb", [1, 3])
@pytest.mark.parametrize("ragged", [True, False])
@pytest.mark.parametrize("n_y", [1, 3])
def test_wd_chain_through_the_atmosphere_table_is_the_forward_model(n_carb, ragged, n_y):
    pack = synth.make_pack("dsed", n_filt=5, n_y=n_y, n_feh=4, n_age=8, n_eep=90, ragged=ragged)
    pack.update(synth.make_wd_tables(5, n_carb=n_carb, ragged=ragged))
    for k in ("wc_n_age", "wc_offset"):
        if not ragged:
            pack.pop(k, None)
    par = synth.default_params(pack)
    par[abi.P_CARBONICITY] = 0.45
    for pop in ((0, 1) if n_y > 1 else (0,)):
        par[abi.P_Y2] = par[abi.P_Y] + 0.01
        iso = synth.derive_isochrone(pack, par[abi.P_LOGAGE], par[abi.P_FEH], par[abi.P_Y2 if pop else abi.P_Y])
        tip = iso[1][-1]
        m = np.linspace(tip * 1.001, pack["m_wd_up"], 300)
        for wd_type in (0, 1):
            wt = np.full(len(m), wd_type)
            want = synth.forward_mags(pack, par, m, np.zeros(len(m)), wt, pop=pop)
            wdm, prec, cool, lteff, logg = wd_check.wd_chain(pack, par, m, pop=pop)
            died = prec < par[abi.P_LOGAGE]
            assert died.sum() > 200 and np.all(cool[~died] == 0) and np.all(lteff[~died] == 0) and np.all(logg[~died] == 0)
            got = wd_check.apparent(pack, par, wd_check.atmosphere_mags(pack, lteff[died], logg[died], wt[died]))
            np.testing.assert_allclose(got, want[died], rtol=1e-13, atol=1e-13)
            np.testing.assert_array_equal(want[~died], wd_check.apparent(pack, par, np.full((int((~died).sum()), 5), -4.0)))
            np.testing.assert_allclose(wdm, synth._ifmr(pack, par, m), rtol=0, atol=0)
            np.testing.assert_allclose(cool[died], np.log10(10.0 ** par[abi.P_LOGAGE] - 10.0 ** prec[died]), rtol=1e-15)


def test_header_library_and_binding_have_the_new_calls():
    header = open(os.path.join(ROOT, "include", "base9_hip.h")).read()
    for name in ("b9_sample_wd_mass", "b9_n_wd_stars"):
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in abi.ABI_SYMBOLS
    assert "#define B9_ABI_VERSION 6" in header
    lib = abi.load_hip_library()
    assert lib.b9_sample_wd_mass.argtypes is not None and len(lib.b9_sample_wd_mass.argtypes) == 14
    assert lib.b9_n_wd_stars.argtypes is not None
    out = subprocess.run(["nm", "-D", "--defined-only", abi.HIP_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"b9_sample_wd_mass", "b9_n_wd_stars"} <= exported


def _device_asm():
    spec = importlib.util.spec_from_file_location("check_async_sloads", os.path.join(ROOT, "tools", "check_async_sloads.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    return chk.device_asm()


def test_every_instance_is_in_the_code_object_and_the_star_kernel_has_no_scratch():
    """Per kernel, from the generated gfx950 assembly: the kernel descriptor's private segment size and the scratch
    instructions in its body (what tools/kernel_resources.py reports).  The table kernel runs the long WD chain once per
    node and is only reported, as k_marg_wd_table is."""
    scratch, instrs, cur = {}, {}, None
    for line in open(_device_asm()):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            continue
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            cur = m.group(1)
            continue
        m = re.match(r"\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", line)
        if m and cur:
            scratch[cur] = int(m.group(1))
        elif cur and ("scratch_load" in line or "scratch_store" in line):
            instrs[cur] = instrs.get(cur, 0) + 1
    # Itanium names: k_wd_node_table<NFP> = _Z15k_wd_node_tableILi<NFP>E..., k_wd_sample<NFP, NPOPS> = _Z11k_wd_sampleILi<NFP>ELi<NPOPS>E...
    for nfp in (4, 8, 16):
        tab = [k for k in scratch if k.startswith("_Z15k_wd_node_tableILi%dEE" % nfp)]
        assert len(tab) == 1, (nfp, tab)
        print(f"k_wd_node_table<{nfp}>: scratch {scratch[tab[0]]} B/lane, {instrs.get(tab[0], 0)} scratch instructions")
        for pops in (1, 2):
            smp = [k for k in scratch if k.startswith("_Z11k_wd_sampleILi%dELi%dEE" % (nfp, pops))]
            assert len(smp) == 1, (nfp, pops, smp)
            assert scratch[smp[0]] == 0 and instrs.get(smp[0], 0) == 0, (smp[0], scratch[smp[0]], instrs.get(smp[0], 0))


def test_shared_res_reader(tmp_path):
    """b9h_read_res_rows = b9h::read_res_rows: leading '#' lines, header -> columns, unknown column -> error, stage filter,
    malformed data lines skipped, parameters that are not columns taken from the starting row."""
    start = np.arange(12, dtype=np.float64) + 100.0
    p = str(tmp_path / "c.res")
    body = ("logAge FeH modulus absorption logPost stage\n"
            "9.1 -0.1 10.0 0.10 -5.0 1\n"
            "9.2 -0.2 10.1 0.11 -4.0 3\n"
            "9.25 -0.25 10.15 0.115 -4.5 2\n"
            "garbage line\n"
            "9.3 -0.3 10.2 0.12 -3.0 3\n"
            "9.4 -0.4 10.3\n")
    open(p, "w").write("# base9_hip ABI 6; mode=givenMass\n# a second comment\n" + body)
    rows = hostlib.read_res_rows(p, start, 3)
    assert rows.shape == (2, 12)
    for k, col in ((abi.P_LOGAGE, [9.2, 9.3]), (abi.P_FEH, [-0.2, -0.3]), (abi.P_MOD, [10.1, 10.2]), (abi.P_ABS, [0.11, 0.12])):
        assert list(rows[:, k]) == col
    others = [k for k in range(12) if k not in (abi.P_LOGAGE, abi.P_FEH, abi.P_MOD, abi.P_ABS)]
    assert np.array_equal(rows[:, others], np.tile(start[others], (2, 1)))
    assert hostlib.read_res_rows(p, start, 1).shape == (1, 12) and hostlib.read_res_rows(p, start, 2)[0, abi.P_LOGAGE] == 9.25
    assert hostlib.read_res_rows(p, start, 7).shape == (0, 12)
    open(p, "w").write(body)                                            # no comment line: the same rows
    assert np.array_equal(hostlib.read_res_rows(p, start, 3), rows)
    open(p, "w").write(body.replace("modulus", "modulusX"))
    with pytest.raises(hostlib.HostError, match="unknown column 'modulusX'"):
        hostlib.read_res_rows(p, start, 3)
    open(p, "w").write("# only a comment\n")
    with pytest.raises(hostlib.HostError, match="is empty"):
        hostlib.read_res_rows(p, start, 3)
    open(p, "w").write("logPost stage\n")
    with pytest.raises(hostlib.HostError, match="malformed header"):
        hostlib.read_res_rows(p, start, 3)
    with pytest.raises(hostlib.HostError, match="cannot read"):
        hostlib.read_res_rows(str(tmp_path / "absent.res"), start, 3)
