"""Mesh cross-sections on the device against exact cuts: the cases of tests/test_section_exact_host.py through
``mm.mesh_cross_sections``, equal to the checker bit for bit (``same_as_checker``), with E1 (points on their mesh edge),
E2 (points on the plane), E3 (topology, the crossed set) and E8 (the origin moves nothing but the selection) asserted on
what the device returned -- and, since the measures come with it, E4 to E7 as well.  Once with the default segment
buffer and once with a buffer one record short, so the second attempt sees these inputs too.  A ``vessel_profile`` along
the thin arm, 1 000 radii from the wide one, against the exact areas of its own polygons."""
import math

import numpy as np
import pytest

import section_exact as Q
from mm_checkers import mesh_sections as X
from test_gpu_section import same_as_checker
from test_section_exact_host import (C3, EPS, NAMES, cases, checked, judge, origin_moves_nothing_but_the_selection)
from test_section_host import same_arrays

import multimoda_rs_amd as mm

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", NAMES)
def test_exact_cut_on_the_device(engine, name):
    v, f, o, n = cases()[name].args()
    got = same_as_checker(mm.mesh_cross_sections((v, f), o, n, engine=engine), checked(name), (v, f), o, n)
    assert got.report["attempts"] == 1 and got.report["n_segments"] > 0
    judge(name, got)
    if name.startswith("corner_loops"):
        origin_moves_nothing_but_the_selection(name, got)
    # one record short: the call is repeated with the count, and nothing differs
    again = mm.mesh_cross_sections((v, f), o, n, max_segments=got.report["n_segments"] - 1, engine=engine)
    assert again.report["attempts"] == 2 and again.report["n_segments"] == got.report["n_segments"]
    same_arrays(again, checked(name))
    judge(name, again, which=("E1", "E2", "E3"))
    if name.startswith("corner_loops"):
        origin_moves_nothing_but_the_selection(name, again)


def test_profile_of_the_thin_arm_far_from_the_wide_one(engine):
    c = cases()["far_origin_1000"]
    xs = 0.5 + 0.25 * np.arange(13)
    xyz = np.stack([xs, np.full(13, 1000.0), np.full(13, 0.25)], 1)
    cl = mm.Centerline.from_arrays(xyz, np.tile([1.0, 0.0, 0.0], (13, 1)), radius=0.02, branch_id=0)
    prof = mm.vessel_profile((c.v, c.f), cl, engine=engine)
    assert prof.report["n_stations"] == 13 and prof.report["n_missing"] == 0
    n = Q.fr([1.0, 0.0, 0.0])
    worst = 0.0
    for k, ct in enumerate(prof.contours):
        pts = ct.points.tolist()
        m, D = len(pts), math.sqrt(sum((max(p[a] for p in pts) - min(p[a] for p in pts)) ** 2 for a in range(3)))
        exact = Q.signed_area(Q.fr_rows(pts), n)
        err = float(abs(Q.F(float(prof.table[k, 2])) - exact))
        worst = max(worst, err / (m * EPS * D * D))
        assert m == 20 and exact > 0 and err <= C3 * m * EPS * D * D, (k, err)
        # the arm's vertices are stored at y ~ 1000, each within 2^-44 of its place: 2 sqrt(2) 2^-44 / 0.02 of the area
        assert abs(prof.table[k, 2] - 5.0 * 0.02 ** 2 * math.sin(2.0 * math.pi / 10.0)) <= 2e-11 * prof.table[k, 2]
        assert np.abs(prof.sections.contour_centroid[prof.sections.selected[k]] - [xs[k], 1000.0, 0.25]).max() <= 4.0 * EPS * 1000.0
    print("thin arm profile: worst E5 %.3g of %g" % (worst, C3))
    assert X.same_bits(prof.table[:, 2], prof.sections.contour_area[prof.sections.selected])
