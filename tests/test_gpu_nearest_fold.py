"""k_slice_nearest (csrc/mm_slice_kernels.hip) and k_cl_morph (csrc/mm_morph_kernels.hip) run one fold
(csrc/mm_point_device.h) from two start values: the slice rule starts at d_0, the morph rule at DBL_MAX.  The same 257
points and 513 targets go through both, with targets on which the two rules part, so a fold handed the other kernel's
start value fails here.  Results against the checkers of tests/mm_checkers."""
import numpy as np
import pytest

from mm_checkers import discretize as DZ
from mm_checkers import scale_coronary as SC

import multimoda_rs_amd as mm
from test_gpu_discretize import device_nearest, same
from test_gpu_morph import cl_of

pytestmark = pytest.mark.gpu

N_PTS, N_TGT, TIE, INF_PT = 257, 513, 511, 100
NEAR_TIE = [3, 200, 256]          # points that sit next to the tied targets 511 == 512


def case():
    r = np.random.default_rng(2024)
    tgt = r.uniform(-10, 10, (N_TGT, 3))
    tgt[TIE] = tgt[TIE + 1] = (30.0, 30.0, 30.0)               # an exact tie across the tile boundary of 512
    pts = r.uniform(-10, 10, (N_PTS, 3))
    pts[NEAR_TIE] = tgt[TIE] + r.normal(scale=0.01, size=(len(NEAR_TIE), 3))
    pts[INF_PT, 1] = np.inf                                    # every distance is inf or NaN: none below DBL_MAX
    nan0 = tgt.copy()
    nan0[0, 2] = np.nan                                        # d_0 is NaN for every point
    far0 = tgt.copy()
    far0[0] = (-500.0, 0.0, 0.0)                               # the same targets with a target 0 no point is near
    normals = r.normal(size=(N_TGT, 3))
    return pts, nan0, far0, normals / np.linalg.norm(normals, axis=1, keepdims=True)


def run_both(engine, pts, tgt, normals, adj=0.5):
    anc = np.concatenate([tgt, normals], 1)
    (si, sq), = device_nearest(engine, [(pts, anc)])
    wi, wq = DZ.nearest_project(pts, anc)
    assert np.array_equal(si, wi) and same(sq, wq)
    (mq, mi), = mm.ccta.centerline_morph_batch([(cl_of(tgt), pts, adj)], engine)
    want, idx = SC.diameter_morphing(tgt, SC.tuples(pts), adj)
    assert mi.tolist() == idx == SC.nearest_indices(tgt, pts).tolist()
    assert same(mq, np.array(want))
    return si, mi


def test_nan_target_0_pins_the_slice_rule_and_never_wins_the_morph_rule(engine):
    pts, nan0, _, normals = case()
    si, mi = run_both(engine, pts, nan0, normals)
    assert (si == 0).all()                                     # best = NaN: no d_j compares below it
    finite = np.arange(N_PTS) != INF_PT
    assert (mi[finite] != 0).all()                             # a NaN d_0 is never below DBL_MAX
    assert mi[INF_PT] == 0                                     # nothing below DBL_MAX: the start index stays
    assert mi[NEAR_TIE].tolist() == [TIE] * len(NEAR_TIE)      # 511 == 512: the lower index


def test_tie_across_the_tile_boundary_keeps_511_under_both_rules(engine):
    pts, _, far0, normals = case()
    si, mi = run_both(engine, pts, far0, normals)
    assert si[NEAR_TIE].tolist() == mi[NEAR_TIE].tolist() == [TIE] * len(NEAR_TIE)
    finite = np.arange(N_PTS) != INF_PT
    assert np.array_equal(si[finite], mi[finite]) and (si[finite] != 0).all()
    assert si[INF_PT] == 0 and mi[INF_PT] == 0                 # d_0 = inf is never beaten; nothing below DBL_MAX
