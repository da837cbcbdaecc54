"""What the eight programs over a saved chain share below their mains (base_amd/host/b9chain.hpp), on the CPU:
tests/host/chain_cli_check.cpp, a stand-alone program built here from b9host.cpp and b9chain.cpp alone with
g++ -fsanitize=address,undefined and run as a child process.  It exits non-zero at the first violated line:

  the row loop      for 1, 255, 256, 257 and 513 rows the batches tile [0, n_rows) in order, none empty, only the first at row 0
  the grid          starSummary / massFunction / starIntervals / photResiduals / modelScore: defaults 1 population and 4 x 4 nodes,
                    the section's key before sampleMass's before 4, nPops 0 and 3 and a grid of 0 refused with the present messages
  nMassNodes        0 and 2147483648 refused; wdSummary's falls back to sampleWDMass's, then 512
  the flag tables   a program's short flags set its own keys on its command line only; the long spellings stay everyone's
  the table writer  %.0f, %ld, %.6f and %.17g columns, with and without a label column, a stride wider than the columns, no lines,
                    an unwritable path

This is where starSummary's and wdSummary's settings are checked without a GPU: they have no export in libbase9host."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chain_cli_check_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "chain_cli_check")
    host = os.path.join(ROOT, "base_amd", "host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "host", "chain_cli_check.cpp"), os.path.join(host, "b9host.cpp"),
           os.path.join(host, "b9chain.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-3000:]
    work = tmp_path / "work"
    work.mkdir()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(work)], capture_output=True, text=True, env=env, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "chain_cli_check: ok" in r.stdout and "runtime error" not in r.stderr
