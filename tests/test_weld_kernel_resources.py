"""The mesh assembly kernels (csrc/mm_weld_kernels.hip), read from the compiler's resource remarks (no GPU): every
kernel is built (its file is in SOURCES), spills nothing, uses no scratch and reaches at least 4 waves per SIMD; the
volume is summed without float atomics and nothing is written in assembly."""
import os
import re
import shutil

import pytest

from test_morph_kernel_resources import HIPCC, ROOT, _compile, _flags

KERNELS = ("k_weld_mark", "k_weld_vertex_insert", "k_weld_vertex_rep", "k_weld_vmap", "k_weld_face_insert",
           "k_weld_face_rep", "k_weld_edge_insert", "k_weld_link_init", "k_weld_hook", "k_weld_jump", "k_weld_flip",
           "k_weld_edge_report", "k_weld_terms", "k_weld_pair_sum", "k_weld_reverse")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_weld_kernels_spill_nothing_and_keep_occupancy(tmp_path):
    b = _flags()
    assert "mm_weld_kernels.hip" in b.SOURCES and "mm_stitch.cpp" in b.SOURCES
    src = os.path.join(ROOT, "multimoda-rs_amd", "csrc", "mm_weld_kernels.hip")
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
    assert not re.search(r"\bglobal_atomic_(add|pk_add|min|max)_f(32|64)\b", text)
    assert "-ffp-contract=off" in b.FLAGS                              # the volume terms are unfused
    for k in ("k_weld_terms", "k_weld_pair_sum"):                      # (the f64 -> int64 conversion of the keys uses one)
        body = re.search(r"^(_ZN2mm\d+" + k + r"\w*):[^\n]*\n(.*?)^\.Lfunc_end", text, flags=re.S | re.M).group(2)
        assert "v_add_f64" in body and not re.search(r"v_fma\w*_f64", body), k
    assert not re.search(r"\basm\b", open(src).read())
