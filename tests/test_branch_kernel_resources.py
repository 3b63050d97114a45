"""The branch mask kernel (csrc/mm_branch_kernels.hip), read from the compiler's resource remarks (no GPU): it is built
(its file and its host side are in SOURCES), spills nothing, uses no scratch, keeps one LDS tile of 32-byte centerline
points far inside the 160 KB of a CU (so several blocks share one) and reaches at least 4 waves per SIMD; its distances
are unfused f64, its mask leaves by a vector store, and it needs neither atomics nor assembly."""
import os
import re
import shutil

import pytest

from test_morph_kernel_resources import HIPCC, ROOT, _compile, _flags

LDS_PER_CU = 160 * 1024


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_branch_mask_kernel_spills_nothing_and_fits_lds(tmp_path):
    b = _flags()
    for f in ("mm_branch_kernels.hip", "mm_branch.cpp", "mm_cl_branches.cpp"):
        assert f in b.SOURCES, f
    src = os.path.join(ROOT, "multimoda-rs_amd", "csrc", "mm_branch_kernels.hip")
    remarks, text = _compile(b, src, tmp_path / "k.s")
    blocks = [blk for blk in re.split(r"remark: Function Name: ", remarks)[1:] if "k_branch_mask" in blk.split()[0]]
    assert len(blocks) == 1
    blk = blocks[0]
    get = lambda key: int(re.search(key + r": (\d+)", blk).group(1))                     # noqa: E731
    assert get("VGPRs Spill") == 0 and get("SGPRs Spill") == 0
    assert get(r"ScratchSize \[bytes/lane\]") == 0
    assert get(r"Occupancy \[waves/SIMD\]") >= 4
    lds = get(r"LDS Size \[bytes/block\]")
    tile = int(re.search(r"kBranchTile = (\d+);", open(src).read()).group(1))
    assert lds == tile * 32 and 4 * lds <= LDS_PER_CU                                   # at least four blocks a CU
    body = re.search(r"^(_ZN2mm\d+k_branch_mask\w*):[^\n]*\n(.*?)^\.Lfunc_end", text, flags=re.S | re.M).group(2)
    assert "-ffp-contract=off" in b.FLAGS
    assert "v_mul_f64" in body and "v_add_f64" in body and not re.search(r"v_fma\w*_f64", body)
    assert re.search(r"\bds_read\w*_b128\b|\bds_load\w*_b128\b", body)                  # a centerline point: 16-byte LDS reads
    assert re.search(r"\bglobal_store_dwordx2\b", body)                                 # the mask: one vector store
    assert not re.search(r"\b(global|flat|ds)_atomic\w*", body)
    assert not re.search(r"\basm\b", open(src).read())
