"""The lumen morphometry kernel (csrc/mm_shape_kernels.hip), read from the compiler's resource remarks and ISA (no GPU):
no spills, no scratch, at least 3 waves per SIMD (the LDS staging allows three workgroups per CU); the distance folds in
unfused v_mul_f64 / v_add_f64; and no more fused f64 operations than the kernel's correctly rounded sqrt and division
expansions account for (per expansion counted on probe kernels built with the same flags; one v_rsq_f64 per sqrt, one
v_div_fixup_f64 per division) -- the bit parity with the reference's unfused arithmetic rests on that."""
import os
import re
import shutil

import pytest

from test_morph_kernel_resources import HIPCC, PROBE, ROOT, _body, _compile, _flags

FUSED = r"\bv_fmac?_f64(?:_e32|_e64)?\b"


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_shape_kernel_spills_nothing_and_fuses_only_div_and_sqrt(tmp_path):
    b = _flags()
    assert "mm_shape_kernels.hip" in b.SOURCES and "mm_shape.cpp" in b.SOURCES
    remarks, text = _compile(b, os.path.join(ROOT, "multimoda-rs_amd", "csrc", "mm_shape_kernels.hip"), tmp_path / "k.s")
    seen = set()
    for blk in re.split(r"remark: Function Name: ", remarks)[1:]:
        name = blk.split()[0]
        get = lambda key: int(re.search(key + r": (\d+)", blk).group(1))
        assert get("VGPRs Spill") == 0 and get("SGPRs Spill") == 0, name
        assert get(r"ScratchSize \[bytes/lane\]") == 0, name
        assert get(r"Occupancy \[waves/SIMD\]") >= 3, name
        seen.add(name)
    assert any("k_contour_measures" in n for n in seen)
    body = _body(text, r"_ZN2mm18k_contour_measures")
    assert "v_add_f64" in body and "v_mul_f64" in body
    n_sqrt = len(re.findall(r"\bv_rsq_f64", body))
    n_div = len(re.findall(r"\bv_div_fixup_f64\b", body))
    assert n_sqrt >= 5 and n_div >= 1                   # both instantiations: far pair, 3-D, 2-D, area; the ratio
    (tmp_path / "probe.hip").write_text(PROBE)
    _, ptext = _compile(b, tmp_path / "probe.hip", tmp_path / "probe.s")
    per_div = len(re.findall(FUSED, _body(ptext, r"_Z11k_probe_div")))
    per_sqrt = len(re.findall(FUSED, _body(ptext, r"_Z12k_probe_sqrt")))
    assert per_div > 0 and per_sqrt > 0
    assert len(re.findall(FUSED, body)) <= n_div * per_div + n_sqrt * per_sqrt
