"""csrc/mm_level_plan.cpp on the CPU (tests/level_plan_host.cpp, a program of its own): compiled by the host compiler with
no ROCm include path -- the planner, its records and its limits need no HIP header -- it plans matrix-pipe, bounded,
exact and empty levels and checks every layout region on a heap block of exactly lvl_bytes.  No GPU, no engine."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_planner_builds_without_hip_and_lays_out_disjoint_regions(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler"
    csrc = os.path.join(ROOT, "multimoda-rs_amd", "csrc")
    exe = str(tmp_path / "level_plan_host")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-pthread", "-I" + csrc,
           os.path.join(csrc, "mm_level_plan.cpp"), os.path.join(ROOT, "tests", "level_plan_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "level_plan_host OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
