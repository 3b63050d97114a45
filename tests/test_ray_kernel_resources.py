"""The ray-triangle kernels of the labelling (csrc/mm_ray_kernels.hip), read from the compiler's resource remarks and
ISA (no GPU): no spills, no scratch, full occupancy, and 1 / a as the correctly rounded f64 division (v_div_scale /
v_div_fmas / v_div_fixup), not a reciprocal shortcut -- the parity with the reference rests on that."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_ray_kernels_spill_nothing_and_divide_exactly(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("mm_build", os.path.join(ROOT, "multimoda-rs_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "mm_ray_kernels.hip" in b.SOURCES
    src = os.path.join(ROOT, "multimoda-rs_amd", "csrc", "mm_ray_kernels.hip")
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
        seen.add("tri" if "k_ray_tri" in name else "fold" if "k_ray_fold" in name else name)
    assert {"tri", "fold"} <= seen
    text = asm.read_text()
    body = text[text.index("k_ray_triEPKdiS1_iiiPNS_10RayPartialE:"):]
    body = body[:body.index("s_endpgm")]
    for op in ("v_div_scale_f64", "v_div_fmas_f64", "v_div_fixup_f64"):
        assert op in body, op
    # the only fused operations are the division's own refinement steps (the file is built with -ffp-contract=off)
    assert len(re.findall(r"\bv_fma(c)?_f64", body)) <= 5
