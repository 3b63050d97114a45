"""The search engine's level planner (csrc/mm_level_plan.cpp, through mm_level_plan_probe) against the plans recorded in
tests/golden/level_plans.json from the engine's staging code as it was before the planner was cut out of it: header,
layout and launch groups field by field, pair descriptors, tables and both work lists as one sha256 an array.  A screen,
a group size, a work item, an offset or one bit of an error bound that moves fails here.  Host only."""
import json
import os

import pytest

import make_golden as G

with open(os.path.join(G.GOLD, "level_plans.json")) as _f:
    DOC = json.load(_f)
CASES = DOC["cases"]
NONE, DIRECT, PACKED, MATRIX, CULL = range(5)
F64 = 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_equals_the_recording(mm, name):
    want = CASES[name]
    got = G.level_plan_entry(want["in"], G.level_plan_probe(want["in"], DOC["lists"]))
    for part in ("header", "layout"):
        assert sorted(got[part]) == sorted(want[part])
        for key in want[part]:
            assert got[part][key] == want[part][key], (name, part, key)
    assert len(got["groups"]) == len(want["groups"])
    for k, (g, w) in enumerate(zip(got["groups"], want["groups"])):
        for key in G.LEVEL_GROUP:
            assert g[key] == w[key], (name, "group", k, key)
    for key in ("pairs", "tables", "work", "work_lb"):
        assert got["sha256"][key] == want["sha256"][key], (name, key)
    assert got == want


def test_recording_reaches_every_branch():
    """Conditions on the FIXTURE: a recording that does not meet them is the wrong recording."""
    assert len(CASES) >= 28
    groups = [g for c in CASES.values() for g in c["groups"]]
    assert {g["screen"] for g in groups} == {NONE, DIRECT, PACKED, MATRIX, CULL}
    assert any(g["multi"] == 1 for g in groups)
    assert any(g["screen"] == MATRIX and g["a_cap"] > 17 for g in groups)           # LDS class 1 stays on the full kernel
    assert {g["nct"] for g in groups if g["screen"] == CULL} >= {2, 3, 7, 17}
    assert {p for c in CASES.values() for p in c["pads"]} >= {0, 2, 4, 8}
    assert CASES["group_auto_full"]["pads"] == [8] and CASES["group_auto_small"]["pads"] == [0]
    bounded = [c["header"] for c in CASES.values() if c["header"]["use_lb"]]
    assert any(h["kept_nct"] > 0 for h in bounded) and any(h["kept_nct"] == 0 and h["lb_stride"] >= 8 for h in bounded)
    assert all(h["W_lb"] > 0 for h in bounded)
    assert not CASES["bounded_mixed"]["header"]["use_lb"] and not CASES["bounded_small"]["header"]["use_lb"]
    assert CASES["bounded_costs"]["layout"]["off_all_costs"] > 0
    # a split per side: taken on both, and refused on one side of a pair that takes the other
    assert 0 not in CASES["split_taken"]["mains"] and len(CASES["split_taken"]["mains"]) == 2
    assert 0 in CASES["split_refused"]["mains"] and len(CASES["split_refused"]["mains"]) == 2
    assert CASES["cull_off"]["mains"] == [0] and CASES["split_off"]["mains"] == [0]
    assert CULL not in {g["screen"] for g in CASES["cull_off"]["groups"]}
    # a level asked for in f32 that fell back to f64, and one that stayed f32 with a set of radius 0
    assert CASES["unsafe_f32"]["in"]["precision"] != F64 and CASES["unsafe_f32"]["header"]["precision"] == F64
    assert CASES["rho_zero"]["header"]["precision"] == CASES["rho_zero"]["in"]["precision"] != F64
    assert CASES["f64"]["trivial"] == 1 and CASES["f64"]["header"]["T"] == 37 + 1 and CASES["f64"]["groups"] == []
    assert not CASES["fast_too_tall"]["header"]["use_fast"]
    assert CASES["slices_beyond"]["header"]["A"] == 0 and CASES["slices"]["header"]["A"] == 2 * 200
    # tables shared by address (one list named by every pair) and by content (equal lists stored twice)
    shared, ptr = CASES["packed_shared"], CASES["packed_shared_ptr"]
    assert len(set(shared["in"]["lists"])) == 2 and len(shared["in"]["lists"]) == 6 and shared["header"]["T"] == 2 * 37
    assert len(ptr["in"]["lists"]) == 1 and ptr["header"]["P"] == 4 and ptr["header"]["T"] == 37


def test_probe_reports_the_count_to_a_short_buffer(mm):
    import ctypes as C
    import numpy as np
    n = C.c_int64(0)
    one = np.zeros(1, dtype=np.int64)
    rc = mm._native.lib().mm_level_plan_probe(0, None, None, None, 0, None, None, None, None, None, None, 0, None, None, None,
                                              None, None, None, 4, 0, 2**31 - 1, 0, 16384, 1, 1, 1, 1, 1, 0,
                                              one.ctypes.data_as(C.c_void_p), 1, C.byref(n))
    assert rc == 0 and n.value == 7 + len(G.LEVEL_HEADER) + len(G.LEVEL_LAYOUT) and one[0] == 0   # an empty level: nothing written
    assert mm._native.lib().mm_level_plan_probe(0, None, None, None, 0, None, None, None, None, None, None, 0, None, None,
                                                None, None, None, None, 9, 0, 1, 0, 0, 1, 1, 1, 1, 1, 0, None, 0,
                                                C.byref(n)) == -2          # MM_ERR_INVALID: no such precision
