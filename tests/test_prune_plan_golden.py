"""The host plans of the pruned searches, against the bytes recorded in tests/golden/prune_plans.json (tests/make_golden.py
prune_plans): every permutation, item list, bound and info value of mm.ccta.nn_plan over tests/nn_worst_cases.py (plain
and morphed sets) and of surface.tri_plan over the meshes of the plan tests in tests/test_surface_host.py, as one sha256
an array.  A change of order, of a tie or of one bit of a bound fails here.  Host only."""
import json
import os

import make_golden


def test_plans_hash_to_the_recorded_bytes(mm):
    with open(os.path.join(make_golden.GOLD, "prune_plans.json")) as f:
        want = json.load(f)
    got = make_golden.prune_plans()
    assert sorted(got) == sorted(want)
    assert len(want) >= 16 + 5 + 5
    for case in sorted(want):
        assert got[case] == want[case], case
