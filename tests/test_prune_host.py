"""csrc/mm_prune.h on the CPU (tests/prune_host.cpp, a program of its own): the slab permutation on empty, equal, NaN,
infinite and overflowing keys, the box on NaN coordinates, box_lb2 against the four-operation formula bit for bit, and
the nearest-first order on tied bounds.  The header includes no HIP and no engine header: the compile line has neither.
No GPU, no engine."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_permutation_box_bound_and_order(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "prune_host")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I" + os.path.join(ROOT, "multimoda-rs_amd", "csrc"),
           os.path.join(ROOT, "tests", "prune_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "prune_host OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
