"""The culled screen's run table on the CPU (tests/cull_runs_host.cpp, a program of its own next to csrc/mm_level_plan.cpp,
built by the host compiler with no ROCm include path): a config3-shaped plan (4 x 511 pairs of 23 items), a plan of one
pair, plans below the 16-round limit, pairs of 1, 2 and 23 items mixed and a plan of two launch groups, each with
ScreenOptions::screen_run automatic, off and forced to 2, 3, 5, 23 and 64.  Every item in exactly one run in list order, no
run across a pair or a launch group, forced sizes honoured up to the pair's items, automatic sizes that only fall along the
list and end in single items, no table below the limit.  No GPU, no engine."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_run_table_properties(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler"
    csrc = os.path.join(ROOT, "multimoda-rs_amd", "csrc")
    exe = str(tmp_path / "cull_runs_host")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-pthread", "-I" + csrc,
           os.path.join(csrc, "mm_level_plan.cpp"), os.path.join(ROOT, "tests", "cull_runs_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0 and "cull_runs_host OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
