"""CCTA mesh morphing on the device (csrc/mm_morph_kernels.hip): the moved points bit for bit against the oracle's
diameter_morphing and the nearest indices against the Python checker (tests/mm_checkers/scale_coronary.py), with the
tie, inf / NaN and empty-job rules; a batch of jobs against the jobs run one by one; label_anomalous_region and three
morph + sync rounds end to end on the labelled synthetic take-off mesh against the checker; and mm.scale on placed
frames with walls."""
import math

import numpy as np
import pytest

from mm_checkers import scale_coronary as SC

import multimoda_rs_amd as mm

pytestmark = pytest.mark.gpu
N = mm._native


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same(a, b):
    """Bit for bit, except that a NaN only has to be a NaN (its sign and payload are the hardware's)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a[~na]), bits(b[~nb]))


def cl_of(xyz):
    """A centerline of the given points (only their coordinates are read here; any count, 0 and 1 included)."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    a = np.zeros(xyz.shape[0], dtype=mm.centerline.CL_DTYPE)
    a["x"], a["y"], a["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return mm.Centerline(a)


def as_tuples(res):
    return {k: (SC.tuples(v) if k != "mesh" else v) for k, v in res.items()}


def random_case(seed, n_pts, n_cl):
    r = np.random.default_rng(seed)
    c = np.cumsum(r.normal(scale=0.15, size=(n_cl, 3)), axis=0)
    p = c[r.integers(0, n_cl, n_pts)] + r.normal(scale=2.0, size=(n_pts, 3))
    return c, p, float(r.uniform(-1.5, 1.5))


@pytest.mark.parametrize("n_cl", [1, 7, 511, 512, 513, 1100])
def test_morph_bitwise_vs_oracle_and_checker(engine, n_cl):
    from oracle import oracle_ccta as occ
    from helpers import to_oracle_cl
    from oracle import oracle_cl as ocl
    c, p, adj = random_case(n_cl, 700, n_cl)
    cl = cl_of(c)
    (got, near), = mm.ccta.centerline_morph_batch([(cl, p, adj)], engine)
    want = occ.diameter_morphing(to_oracle_cl(ocl, cl), p, adj)
    assert np.array_equal(bits(got), bits(want))
    assert near.tolist() == SC.nearest_indices(cl.xyz(), p).tolist()


def test_many_jobs_in_one_launch_equal_jobs_one_by_one(engine):
    jobs = []
    for k, (n_pts, n_cl) in enumerate([(300, 40), (0, 5), (1, 600), (1025, 513), (257, 1), (0, 0), (90, 1030)]):
        c, p, adj = random_case(50 + k, n_pts, max(n_cl, 1))
        jobs.append((cl_of(c[:n_cl]) if n_cl else cl_of(np.zeros((0, 3))), p, adj))
    batch = mm.ccta.centerline_morph_batch(jobs, engine)
    for job, (bo, bn) in zip(jobs, batch):
        (so, sn), = mm.ccta.centerline_morph_batch([job], engine)
        assert np.array_equal(bits(bo), bits(so)) and np.array_equal(bn, sn)
        if len(job[0]):
            want, idx = SC.diameter_morphing(job[0].xyz(), SC.tuples(job[1]), job[2])
            assert same(bo, np.array(want).reshape(-1, 3)) and bn.tolist() == idx


def test_ties_centerline_points_and_special_values(engine):
    c = np.array([[0.0, 0, 0], [2.0, 0, 0], [4.0, 0, 0], [math.nan, 0, 0], [1e300, 0, 0]])
    p = np.array([[1.0, 3.0, 0.0],            # equidistant from 0 and 1: the lowest index
                  [3.0, -1.0, 0.0],           # equidistant from 1 and 2
                  [2.0, 0.0, 0.0],            # on centerline point 1: does not move
                  [math.inf, 0.0, 0.0],       # no distance below DBL_MAX: index 0; |v| = inf: NaN x
                  [math.nan, 1.0, 0.0],       # NaN distances never win: index 0; NaN norm: stays
                  [0.0, math.inf, 0.0],       # distance inf to all: index 0
                  [-0.0, -0.0, 5.0]])
    cl = cl_of(c)
    (got, near), = mm.ccta.centerline_morph_batch([(cl, p, 0.75)], engine)
    want, idx = SC.diameter_morphing(cl.xyz(), SC.tuples(p), 0.75)
    assert near.tolist() == idx == [0, 1, 1, 0, 0, 0, 0]
    assert same(got, np.array(want))
    assert np.array_equal(bits(got[2]), bits(p[2]))
    assert np.isnan(got[4, 0]) and got[4, 1:].tolist() == [1.0, 0.0]


def test_empty_job_and_empty_centerline(engine):
    cl = cl_of(np.zeros((0, 3)))
    assert [o.shape for o, _ in mm.ccta.centerline_morph_batch([(cl, np.zeros((0, 3)), 1.0)], engine)] == [(0, 3)]
    with pytest.raises(RuntimeError):
        mm.ccta.centerline_morph_batch([(cl, np.ones((3, 3)), 1.0)], engine)


def test_scale_region_moves_every_duplicated_vertex(engine):
    c = np.stack([np.zeros(20), np.zeros(20), np.arange(20.0)], 1)
    v = np.array([[1.0, 0, 3], [0, 2.0, 7], [1.0, 0, 3], [-0.0, 2.0, 7], [5.0, 5, 5]])
    f = np.array([[0, 1, 2]])
    out = mm.scale_region_centerline_morphing((v, f), [(1.0, 0.0, 3.0), (0.0, 2.0, 7.0)], cl_of(c), 0.5, engine=engine)
    assert out[1] is f and np.array_equal(v[4], out[0][4])
    assert out[0][:4].tolist() == [[1.5, 0, 3], [0, 2.5, 7], [1.5, 0, 3], [0, 2.5, 7]]
    assert v[0].tolist() == [1.0, 0, 3]                                            # the input is not modified


def test_label_anomalous_region_and_three_rounds_end_to_end(engine):
    v, f, ca, cr, cll, _ = mm.synth.synthetic_takeoff_mesh()
    cla, clr, cl_l = cl_of(ca), cl_of(cr), cl_of(cll)
    res = mm.label_geometry((v, f), cla, clr, cl_l, acute_takeoff_rca=True, engine=engine)
    want = as_tuples(res)
    frames = cr[20:52:2]                                                           # centroids of the imaged section
    split = mm.find_points_by_cl_region(clr, frames, res["rca_points"], engine=engine)
    got = mm.label_anomalous_region(clr, frames, res, engine=engine)
    assert got is res
    SC.label_anomalous_region(split, v, f, want)
    for k in ("rca_points", "proximal_points", "distal_points", "anomalous_points", "aorta_points"):
        assert np.array_equal(bits(got[k]), bits(np.array(want[k]).reshape(-1, 3))), k
    assert len(got["anomalous_points"]) > 0 and len(got["distal_points"]) + len(got["proximal_points"]) > 0

    scal = (0.3, -0.2, 0.25)                                                       # proximal, distal, aortic
    r = got
    m = mm.scale_region_centerline_morphing(r["mesh"], r["distal_points"], clr, scal[1], engine=engine)
    r = mm.sync_results_to_mesh(r, r["mesh"], m)
    region = np.concatenate([r["aorta_points"], np.asarray(r["rca_removed_points"]).reshape(-1, 3)])
    m = mm.scale_region_centerline_morphing(r["mesh"], region, cla, scal[2], engine=engine)
    r = mm.sync_results_to_mesh(r, r["mesh"], m)
    m = mm.scale_region_centerline_morphing(r["mesh"], r["proximal_points"], clr, scal[0], engine=engine)
    r = mm.sync_results_to_mesh(r, r["mesh"], m)
    want["mesh"] = SC.tuples(v)
    w = SC.scale_rounds(want, cr, ca, *scal)
    assert np.array_equal(bits(r["mesh"][0]), bits(np.array(w["mesh"])))
    assert not np.array_equal(r["mesh"][0], v) and r["mesh"][1] is f
    for k in ("aorta_points", "rca_points", "lca_points", "rca_removed_points", "proximal_points", "distal_points",
              "anomalous_points"):
        assert np.array_equal(bits(np.asarray(r[k]).reshape(-1, 3)), bits(np.array(w[k]).reshape(-1, 3))), k


def test_scale_on_frames_with_walls(engine, mm, oracle):
    from test_golden_and_api import _array_input
    from oracle import oracle_ccta as occ, oracle_cl as ocl
    from helpers import to_oracle_cl
    dia = _array_input(mm, n_frames=16, n_points=120, thickness=0.9, seed=3)
    sys_ = _array_input(mm, n_frames=14, n_points=120, thickness=1.1, seed=4)
    sys_.diastole = False
    pair, _ = mm.from_array_singlepair(dia, sys_, step_rotation_deg=1.0, range_rotation_deg=20.0, engine=engine)
    a, b = pair.geom_a, pair.geom_b
    case = mm.synth.synthetic_centerline_case(geometry=a, n_ccta=2500, seed=9, true_rotation_deg=21.0, true_index=7)
    geo = mm.GeometryPair(case["geometry"], b, pair.label)
    aligned, _, _ = mm.align_combined(case["centerline"], geo, case["main_ref_pt"], case["ccw_ref_pt"],
                                      case["cw_ref_pt"], case["points"], angle_range_deg=6.0,
                                      align_wall_anomalous=True, engine=engine)
    g = aligned.geom_a
    rcl, _ = mm.preprocess_centerline(case["centerline"], a)
    cla = cl_of(rcl.xyz() + np.array([6.0, 0.0, 0.0]))
    cloud = mm.adjust_diameter_centerline_morphing_simple(rcl, g.lumen, 0.4)
    aorta = cloud[::5] + np.array([6.0, 0.0, 0.0])
    verts = np.concatenate([cloud, aorta])
    faces = np.arange(3 * (verts.shape[0] // 3)).reshape(-1, 3)
    n = cloud.shape[0]
    res = {"mesh": (verts, faces), "anomalous_points": cloud, "distal_points": cloud[: n // 4],
           "proximal_points": cloud[-n // 4:], "rca_removed_points": cloud[n // 3: n // 3 + 40], "aorta_points": aorta,
           "rca_points": cloud}
    out = mm.scale(dict(res), rcl, cla, g, engine=engine)
    prox, dist = mm.find_distal_and_proximal_scaling(g, rcl, res, engine=engine)
    n4 = int(math.ceil(0.25 * n))
    F = g.n_frames
    assert (prox, dist) == occ.diameter_optimization(cloud, n4, n4, to_oracle_cl(ocl, rcl), g.lumen[:g.lumen_off[2]],
                                                     g.lumen[g.lumen_off[F - 3]:])
    ao = mm.find_aorta_scaling(g, cla, res, engine=engine)
    assert ao == occ.aortic_diameter_optimization(res["rca_removed_points"], mm.ccta._extract_wall_from_frames(g),
                                                  to_oracle_cl(ocl, cla))[0]
    want = as_tuples(res)
    want["mesh"] = SC.tuples(verts)
    w = SC.scale_rounds(want, rcl.xyz(), cla.xyz(), prox, dist, ao)
    assert np.array_equal(bits(out["mesh"][0]), bits(np.array(w["mesh"])))
    for k in ("aorta_points", "rca_points", "rca_removed_points", "proximal_points", "distal_points",
              "anomalous_points"):
        assert np.array_equal(bits(np.asarray(out[k]).reshape(-1, 3)), bits(np.array(w[k]).reshape(-1, 3))), k
    assert not np.array_equal(out["mesh"][0], verts)
