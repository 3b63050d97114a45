"""The mesh trimming kernels (csrc/mm_trim_kernels.hip), read from the compiler's resource remarks (no GPU): every
kernel is built (its file is in SOURCES), spills nothing, uses no scratch and reaches at least 4 waves per SIMD."""
import os
import re
import shutil

import pytest

from test_morph_kernel_resources import HIPCC, ROOT, _compile, _flags

KERNELS = ("k_trim_faces", "k_trim_edge_insert", "k_trim_edge_compact", "k_trim_tile_count", "k_trim_tile_scan",
           "k_trim_index", "k_trim_gather", "k_trim_remap", "k_trim_clear")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_trim_kernels_spill_nothing_and_keep_occupancy(tmp_path):
    b = _flags()
    assert "mm_trim_kernels.hip" in b.SOURCES and "mm_trim.cpp" in b.SOURCES
    remarks, text = _compile(b, os.path.join(ROOT, "multimoda-rs_amd", "csrc", "mm_trim_kernels.hip"), tmp_path / "k.s")
    seen = set()
    for blk in re.split(r"remark: Function Name: ", remarks)[1:]:
        name = blk.split()[0]
        get = lambda key: int(re.search(key + r": (\d+)", blk).group(1))                 # noqa: E731
        assert get("VGPRs Spill") == 0 and get("SGPRs Spill") == 0, name
        assert get(r"ScratchSize \[bytes/lane\]") == 0, name
        assert get(r"Occupancy \[waves/SIMD\]") >= 4, name
        seen.add(name)
    for k in KERNELS:
        assert any(k in n for n in seen), k
    # the compaction appends with one returning atomic per wave, and no float atomics anywhere
    assert not re.search(r"\bglobal_atomic_(add|pk_add|min|max)_f(32|64)\b", text)
    assert not re.search(r"\basm\b", open(os.path.join(ROOT, "multimoda-rs_amd", "csrc", "mm_trim_kernels.hip")).read())
