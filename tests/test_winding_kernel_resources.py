"""The winding-number kernels (csrc/mm_winding_kernels.hip), read from the compiler's resource remarks and ISA (no GPU):
built (the file and its host side are in SOURCES), no spill, no scratch, at least 4 waves per SIMD, one chunk of 9-double
faces in LDS, no inline assembly, and no more fused f64 operations than its six square roots and two divisions expand to
-- the bit parity with the checker's unfused arithmetic rests on that.  The per-face step (csrc/mm_winding_device.h) is
also built as plain host C++ into a program of its own, plain and under ASan + UBSan, and run directly."""
import os
import re
import shutil
import subprocess

import pytest

from test_morph_kernel_resources import FUSED, HIPCC, PROBE, ROOT, _body, _compile, _flags

CSRC = os.path.join(ROOT, "multimoda-rs_amd", "csrc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_winding_kernels_spill_nothing_and_fuse_only_div_and_sqrt(tmp_path):
    b = _flags()
    for f in ("mm_winding_kernels.hip", "mm_winding.cpp"):
        assert f in b.SOURCES, f
    assert "mm_winding_device.h" in b.HEADERS and "-ffp-contract=off" in b.FLAGS
    for name in ("mm_winding_kernels.hip", "mm_winding_device.h"):
        assert not re.search(r"\basm\b|__asm", open(os.path.join(CSRC, name)).read()), name
    remarks, text = _compile(b, os.path.join(CSRC, "mm_winding_kernels.hip"), tmp_path / "k.s")
    blocks = {blk.split()[0]: blk for blk in re.split(r"remark: Function Name: ", remarks)[1:]}
    assert len(blocks) == 2 and any("k_wind_partial" in n for n in blocks) and any("k_wind_join" in n for n in blocks)
    for name, blk in blocks.items():
        get = lambda key: int(re.search(key + r": (\d+)", blk).group(1))                  # noqa: E731
        assert get("VGPRs Spill") == 0 and get("SGPRs Spill") == 0, name
        assert get(r"ScratchSize \[bytes/lane\]") == 0, name
        assert get(r"Occupancy \[waves/SIMD\]") >= 4, name
        assert get(r"LDS Size \[bytes/block\]") == (256 * 9 * 8 if "k_wind_partial" in name else 0), name
        print(name, {k: get(k) for k in ("VGPRs", "SGPRs", r"Occupancy \[waves/SIMD\]", r"LDS Size \[bytes/block\]")})
    body = _body(text, r"_ZN2mm14k_wind_partial")
    assert "v_add_f64" in body and "v_mul_f64" in body and "v_ldexp_f64" in body and "v_frexp_exp_i32_f64" in body
    n_div, n_sqrt = len(re.findall(r"\bv_div_fixup_f64\b", body)), 6               # 2 queries x (1 division, 3 roots)
    assert n_div == 2
    (tmp_path / "probe.hip").write_text(PROBE)
    _, ptext = _compile(b, tmp_path / "probe.hip", tmp_path / "probe.s")
    per_div = len(re.findall(FUSED, _body(ptext, r"_Z11k_probe_div")))
    per_sqrt = len(re.findall(FUSED, _body(ptext, r"_Z12k_probe_sqrt")))
    assert len(re.findall(FUSED, body)) <= n_div * per_div + n_sqrt * per_sqrt
    assert not re.findall(FUSED, _body(text, r"_ZN2mm11k_wind_join"))


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_winding_step_as_host_code_in_a_program_of_its_own(tmp_path, sanitize):
    """tests/winding_device_host.cpp: compiled for the host alone, run directly; nothing sanitised is loaded into Python."""
    cxx = shutil.which("g++") or shutil.which("c++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "winding_device_host")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", *sanitize, "-I" + CSRC,
           os.path.join(ROOT, "tests", "winding_device_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "winding_device_host OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
