"""The mesh smoothing kernels (csrc/mm_smooth_kernels.hip), read from the compiler's resource remarks (no GPU): both new
sources are built (they are in SOURCES), every kernel is there, spills nothing, uses no scratch and reaches at least 4
waves per SIMD; the atomics are integer atomics and nothing is written in assembly."""
import os
import re
import shutil

import pytest

from test_morph_kernel_resources import HIPCC, ROOT, _compile, _flags

KERNELS = ("k_smooth_degree", "k_smooth_scan_count", "k_smooth_scan_tiles", "k_smooth_scan_offsets", "k_smooth_fill",
           "k_smooth_row_sort", "k_smooth_step", "k_smooth_ring_seed", "k_smooth_ring", "k_smooth_disp")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_smooth_kernels_spill_nothing_and_keep_occupancy(tmp_path):
    b = _flags()
    assert "mm_smooth_kernels.hip" in b.SOURCES and "mm_smooth.cpp" in b.SOURCES
    src = os.path.join(ROOT, "multimoda-rs_amd", "csrc", "mm_smooth_kernels.hip")
    remarks, text = _compile(b, src, tmp_path / "k.s")
    seen = {}
    for blk in re.split(r"remark: Function Name: ", remarks)[1:]:
        name = blk.split()[0]
        get = lambda key: int(re.search(key + r": (\d+)", blk).group(1))                 # noqa: E731
        assert get("VGPRs Spill") == 0 and get("SGPRs Spill") == 0, name
        assert get(r"ScratchSize \[bytes/lane\]") == 0, name
        assert get(r"Occupancy \[waves/SIMD\]") >= 4, name
        seen[name] = get("VGPRs")
    for k in KERNELS:
        assert any(re.search(k + r"E", n) or n == k for n in seen), k
    assert len(seen) == len(KERNELS)
    assert not re.search(r"\bglobal_atomic_\w*_f(16|32|64)\b", text)
    assert not re.search(r"\batomic\w*_(f16|f32|f64)\b", text)
    assert not re.search(r"\basm\b", open(src).read())
