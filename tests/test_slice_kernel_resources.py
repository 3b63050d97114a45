"""The nearest-anchor kernel of the vessel discretisation (csrc/mm_slice_kernels.hip), read from the compiler's resource
remarks and ISA (no GPU): no spills, no scratch, at least 4 waves per SIMD, and no fused multiply-add in its body -- the
bit parity with the reference's unfused sq_dist3 and plane projection rests on that."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_slice_kernel_spills_nothing_and_fuses_nothing(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("mm_build", os.path.join(ROOT, "multimoda-rs_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "mm_slice_kernels.hip" in b.SOURCES
    src = os.path.join(ROOT, "multimoda-rs_amd", "csrc", "mm_slice_kernels.hip")
    asm = tmp_path / "k.s"
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", "-x", "hip", *b.FLAGS, "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "multimoda-rs_amd", "csrc"), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-S", src, "-o", str(asm)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = set()
    for blk in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        name = blk.split()[0]
        get = lambda key: int(re.search(key + r": (\d+)", blk).group(1))
        assert get("VGPRs Spill") == 0 and get(r"ScratchSize \[bytes/lane\]") == 0, name
        assert get(r"Occupancy \[waves/SIMD\]") >= 4, name
        seen.add(name)
    assert any("k_slice_nearest" in n for n in seen)
    text = asm.read_text()
    start = re.search(r"^_ZN2mm15k_slice_nearest\S*:", text, re.M)
    assert start
    body = text[start.end():]
    body = body[:body.index("s_endpgm")]
    assert "v_add_f64" in body and "v_mul_f64" in body
    assert not re.findall(r"\bv_fmac?_f64", body)
