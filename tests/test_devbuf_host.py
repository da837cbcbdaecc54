"""Who owns a context's memory (base_amd/csrc/b9_devbuf.h), checked on the CPU: the shipped header, unchanged, under a counting
allocator that fails its N-th call (tests/probes/devbuf_host.cpp, a stand-alone program built here with
g++ -fsanitize=address,undefined and run as a child process).  It walks every failure point of every sequence and exits
non-zero at the first violated line: a failed reserve leaves pointer null AND capacity 0, growth frees the old block once,
a moved-from buffer frees nothing, nothing is live at the end, the upload list frees the block whose copy failed, the work
buffers' and the tree buffers' groups hold what the sizing functions ask for after every step, the carve is ordered, disjoint
and aligned -- the one arena of the four reductions over a saved chain (chain_arena) included: its parts do not overlap, lie
on 8-byte boundaries, `bytes` is the end of the last part, and a call without WD-stage stars, row sums or a tail carves empty
parts; and the one arena of the three calls on a WD mass grid (wd_grid_arena) the same way, at the offsets and totals the draws,
the moments and the bins had from an arena each.

There is no GPU test of these paths on purpose: allocation failures are not provoked on a device, and the tree-buffer defect
this header removed wrote out of bounds.  That defect as arithmetic -- the rule the tree buffers were sized by before:

    n_cand(W, depth) = 2 * W * 2^depth * (2^depth - 1)          parameter rows: B9_NPARAM * n_cand doubles
    reallocate all three candidate buffers  iff  n_cand * n_pops > tree_cand_cap;   then tree_cand_cap = n_cand * n_pops

    step 1: W = 2, n_pops = 2, depth 3:  n_cand = 224,  224 * 2 = 448 > 0      -> parameter rows 224 * 12 doubles, cap = 448
    step 2: W = 4, n_pops = 1, depth 3:  n_cand = 448,  448 * 1 = 448 > 448 ?  no -> nothing reallocated:
            the launch indexes 448 * 12 doubles of parameter rows in a buffer of 224 * 12.

The program drives TreeBufs through exactly these steps and checks capacity >= B9_NPARAM * n_cand after each."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_old_tree_rule_fails_its_second_step():
    """The arithmetic of the docstring, evaluated: the rule keyed on n_cand * n_pops leaves half the parameter rows unallocated."""
    def n_cand(w, depth):
        return 2 * w * (1 << depth) * ((1 << depth) - 1)
    cap_key, par_doubles = 0, 0
    for w, pops, depth in [(2, 2, 3), (4, 1, 3)]:
        if n_cand(w, depth) * pops > cap_key:
            cap_key, par_doubles = n_cand(w, depth) * pops, 12 * n_cand(w, depth)
    assert par_doubles == 224 * 12 and 12 * n_cand(4, 3) == 448 * 12 and par_doubles < 12 * n_cand(4, 3)


def test_devbuf_on_a_counting_allocator(tmp_path):
    exe = str(tmp_path / "devbuf_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-o", exe,
           os.path.join(ROOT, "tests", "probes", "devbuf_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "devbuf_host: ok" in r.stdout
