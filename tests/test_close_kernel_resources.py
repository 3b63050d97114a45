"""The mesh closing kernels (csrc/mm_close_kernels.hip), read from the compiler's resource remarks (no GPU): every
kernel is built (its file is in SOURCES), spills nothing, uses no scratch and reaches at least 4 waves per SIMD; there
are no float atomics (the votes and the counts are integer atomics) and nothing is written in assembly."""
import os
import re
import shutil

import pytest

from test_morph_kernel_resources import HIPCC, ROOT, _compile, _flags

KERNELS = ("k_close_half_edges", "k_close_fan", "k_smooth_vote", "k_smooth_apply", "k_smooth_csr")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_close_kernels_spill_nothing_and_keep_occupancy(tmp_path):
    b = _flags()
    assert "mm_close_kernels.hip" in b.SOURCES and "mm_close.cpp" in b.SOURCES
    src = os.path.join(ROOT, "multimoda-rs_amd", "csrc", "mm_close_kernels.hip")
    remarks, text = _compile(b, src, tmp_path / "k.s")
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
    assert not re.search(r"\bglobal_atomic_\w*_f(16|32|64)\b", text)
    assert not re.search(r"\basm\b", open(src).read())
