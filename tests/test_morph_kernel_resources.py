"""The centerline morphing kernel (csrc/mm_morph_kernels.hip), read from the compiler's resource remarks and ISA (no
GPU): no spills, no scratch, at least 4 waves per SIMD; the distance fold in unfused v_mul_f64 / v_add_f64; the
correctly rounded division expansion (v_div_scale / v_div_fmas / v_div_fixup); and no more fused f64 operations than
three divisions and one sqrt expand to (counted on probe kernels built with the same flags) -- the bit parity with the
reference's unfused arithmetic rests on that."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PROBE = """#include <hip/hip_runtime.h>
__global__ void k_probe_div(const double* a, double* o) { o[threadIdx.x] = a[threadIdx.x] / a[threadIdx.x + 256]; }
__global__ void k_probe_sqrt(const double* a, double* o) { o[threadIdx.x] = sqrt(a[threadIdx.x]); }
"""
FUSED = r"\bv_fmac?_f64\b"


def _flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mm_build", os.path.join(ROOT, "multimoda-rs_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def _compile(b, src, asm):
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", "-x", "hip", *b.FLAGS, "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "multimoda-rs_amd", "csrc"), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-S", str(src), "-o", str(asm)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr, asm.read_text()


def _body(text, sym):
    start = re.search(r"^" + sym + r"\S*:", text, re.M)
    assert start, sym
    body = text[start.end():]
    return body[:body.index("s_endpgm")]


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_morph_kernel_spills_nothing_and_fuses_only_div_and_sqrt(tmp_path):
    b = _flags()
    assert "mm_morph_kernels.hip" in b.SOURCES
    remarks, text = _compile(b, os.path.join(ROOT, "multimoda-rs_amd", "csrc", "mm_morph_kernels.hip"), tmp_path / "k.s")
    seen = set()
    for blk in re.split(r"remark: Function Name: ", remarks)[1:]:
        name = blk.split()[0]
        get = lambda key: int(re.search(key + r": (\d+)", blk).group(1))
        assert get("VGPRs Spill") == 0 and get(r"ScratchSize \[bytes/lane\]") == 0, name
        assert get(r"Occupancy \[waves/SIMD\]") >= 4, name
        seen.add(name)
    assert any("k_cl_morph" in n for n in seen)
    body = _body(text, r"_ZN2mm10k_cl_morph")
    assert "v_add_f64" in body and "v_mul_f64" in body
    for op in ("v_div_scale_f64", "v_div_fmas_f64", "v_div_fixup_f64"):
        assert op in body, op
    assert len(re.findall(r"\bv_div_fixup_f64\b", body)) == 3                 # three divisions, not one reciprocal
    (tmp_path / "probe.hip").write_text(PROBE)
    _, ptext = _compile(b, tmp_path / "probe.hip", tmp_path / "probe.s")
    per_div = len(re.findall(FUSED, _body(ptext, r"_Z11k_probe_div")))
    per_sqrt = len(re.findall(FUSED, _body(ptext, r"_Z12k_probe_sqrt")))
    assert len(re.findall(FUSED, body)) <= 3 * per_div + per_sqrt
