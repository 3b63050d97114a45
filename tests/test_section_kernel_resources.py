"""The plane-cut kernel (csrc/mm_section_kernels.hip), read from the compiler's resource remarks (no GPU): it is built
(its file and its host side are in SOURCES), spills nothing, uses no scratch, keeps exactly one run of 48-byte planes
in LDS and reaches at least 4 waves per SIMD."""
import os
import re
import shutil

import pytest

from test_morph_kernel_resources import HIPCC, ROOT, _compile, _flags


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_section_cut_kernel_spills_nothing_and_keeps_one_plane_run_in_lds(tmp_path):
    b = _flags()
    for f in ("mm_section_kernels.hip", "mm_section.cpp"):
        assert f in b.SOURCES, f
    assert "mm_section_device.h" in b.HEADERS and "-ffp-contract=off" in b.FLAGS
    src = os.path.join(ROOT, "multimoda-rs_amd", "csrc", "mm_section_kernels.hip")
    remarks, _text = _compile(b, src, tmp_path / "k.s")
    blocks = {blk.split()[0]: blk for blk in re.split(r"remark: Function Name: ", remarks)[1:]}
    cut = [blk for name, blk in blocks.items() if "k_section_cut" in name]
    assert len(cut) == 1 and any("k_section_clear" in name for name in blocks)
    get = lambda key: int(re.search(key + r": (\d+)", cut[0]).group(1))                  # noqa: E731
    assert get("VGPRs Spill") == 0 and get("SGPRs Spill") == 0
    assert get(r"ScratchSize \[bytes/lane\]") == 0
    assert get(r"Occupancy \[waves/SIMD\]") >= 4
    run = int(re.search(r"kSectionPlaneRun = (\d+);", open(src).read()).group(1))
    assert run == 64 and get(r"LDS Size \[bytes/block\]") == run * 48
    print("k_section_cut:", {k: get(k) for k in ("VGPRs", "SGPRs", r"Occupancy \[waves/SIMD\]", r"LDS Size \[bytes/block\]")})
