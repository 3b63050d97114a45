"""csrc/mm_stage.h and csrc/mm_point_records.h on the CPU (tests/stage_host.cpp, a program of its own): the 256-byte
carving (take and the typed place) and the staged pass's regions on empty and odd sizes (0, 1, 255, 256, 257), the mesh
scratch layouts of csrc/mm_mesh_layout.h against recorded sizes and offsets, the block work lists, and the record layouts'
static_asserts, which fail the compile.  No GPU, no engine."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_carving_and_staged_pass_regions(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or "/opt/rocm/llvm/bin/clang++"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "stage_host")
    cmd = [cxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
           "-I" + os.path.join(ROOT, "multimoda-rs_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "stage_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "stage_host OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
