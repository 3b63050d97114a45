"""The clip kernels (csrc/mm_clip_kernels.hip), read from the compiler's resource remarks and ISA (no GPU): built (the
file and its host side are in SOURCES, the per-face header in HEADERS), no spill and no scratch in any kernel, no inline
assembly, and no fused f64 instruction in the emit and the count kernels, which run the diagonal test -- the bit parity
with the checker's unfused arithmetic rests on that.  The per-face step (csrc/mm_clip_device.h) is also built as plain
host C++ into a program of its own, plain and under ASan + UBSan, and run directly."""
import os
import re
import shutil
import subprocess

import pytest

from test_morph_kernel_resources import FUSED, HIPCC, ROOT, _body, _compile, _flags

CSRC = os.path.join(ROOT, "multimoda-rs_amd", "csrc")
KERNELS = ("k_clip_init", "k_clip_scatter", "k_clip_sides", "k_clip_union", "k_clip_verdict", "k_clip_orphan", "k_clip_keep", "k_clip_count",
           "k_clip_tile_sum", "k_clip_tile_scan", "k_clip_offsets", "k_clip_vertices", "k_clip_emit", "k_clip_rim")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_clip_kernels_spill_nothing_and_fuse_nothing(tmp_path):
    b = _flags()
    for f in ("mm_clip_kernels.hip", "mm_clip.cpp"):
        assert f in b.SOURCES, f
    assert "mm_clip_device.h" in b.HEADERS and "-ffp-contract=off" in b.FLAGS
    for name in ("mm_clip_kernels.hip", "mm_clip_device.h", "mm_clip.cpp"):
        assert not re.search(r"\basm\b|__asm", open(os.path.join(CSRC, name)).read()), name
    remarks, text = _compile(b, os.path.join(CSRC, "mm_clip_kernels.hip"), tmp_path / "k.s")
    blocks = {blk.split()[0]: blk for blk in re.split(r"remark: Function Name: ", remarks)[1:]}
    assert len(blocks) == len(KERNELS)
    for kernel in KERNELS:
        (name,) = [n for n in blocks if re.search(r"\d" + kernel + "E", n)]
        blk = blocks[name]
        get = lambda key: int(re.search(key + r": (\d+)", blk).group(1))                  # noqa: E731
        assert get("VGPRs Spill") == 0 and get("SGPRs Spill") == 0, name
        assert get(r"ScratchSize \[bytes/lane\]") == 0, name
        assert get(r"Occupancy \[waves/SIMD\]") >= 4, name
        print(kernel, {k: get(k) for k in ("VGPRs", "SGPRs", r"Occupancy \[waves/SIMD\]", r"LDS Size \[bytes/block\]")})
    for kernel in ("k_clip_emit", "k_clip_count", "k_clip_sides"):
        body = _body(text, r"_ZN2mm\d+" + kernel)
        assert "v_mul_f64" in body and "v_add_f64" in body and not re.findall(FUSED, body), kernel
    assert "global_atomic_add_f" not in text and "global_atomic_pk_add" not in text        # no float atomics


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_clip_step_as_host_code_in_a_program_of_its_own(tmp_path, sanitize):
    """tests/clip_device_host.cpp: compiled for the host alone, run directly; nothing sanitised is loaded into Python."""
    cxx = shutil.which("g++") or shutil.which("c++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "clip_device_host")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", *sanitize, "-I" + CSRC,
           os.path.join(ROOT, "tests", "clip_device_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "clip_device_host OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
