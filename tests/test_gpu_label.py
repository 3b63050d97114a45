"""CCTA mesh labelling on the device, bit-exact against the numpy checker (tests/mm_checkers/label_coronary.py): the
ray-triangle pass (csrc/mm_ray_kernels.hip) on random and degenerate inputs and on a synthetic acute take-off, the
radius queries, and label_geometry end to end."""
import numpy as np
import pytest

from mm_checkers import label_coronary as LC

import multimoda_rs_amd as mm
from multimoda_rs_amd.centerline import Centerline

pytestmark = pytest.mark.gpu


def _cl(xyz):
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    return Centerline.from_arrays(xyz, np.zeros_like(xyz))


def _device_occlusion(engine, cc, ca, rng_mm, pts, tris, step=1.0):
    rm, ex = mm.ccta.occluded_point_flags(_cl(cc), _cl(ca), rng_mm, pts, tris, step, engine=engine)
    return rm.astype(bool), set(np.nonzero(ex)[0].tolist())


def _random_scene(seed, nf, n_aorta, n_cor):
    """Big triangles stacked across x (many rays hit >= 3), rays from near x = 0 towards x = 20, plus degenerate
    faces: duplicates of earlier faces (equal t), faces through a ray's origin-to-target line at a vertex or an edge,
    faces parallel to the rays, faces at t just around 1e-8, NaN corners."""
    r = np.random.default_rng(seed)
    ca = np.stack([np.zeros(n_aorta), r.uniform(-1, 1, n_aorta), r.uniform(-1, 1, n_aorta)], 1)
    cc = np.stack([np.full(n_cor, 20.0), r.uniform(-2, 2, n_cor), r.uniform(-2, 2, n_cor)], 1)
    x = r.uniform(0.5, 19.5, nf)
    tris = np.stack([x + r.normal(0, 0.3, nf), r.uniform(-9, -3, nf), r.uniform(-9, -3, nf),
                     x + r.normal(0, 0.3, nf), r.uniform(3, 9, nf), r.uniform(-6, 0, nf),
                     x + r.normal(0, 0.3, nf), r.uniform(-3, 3, nf), r.uniform(3, 9, nf)], 1)
    k = min(nf // 8, 40)
    if k:
        o, d = ca[0], cc[0] - ca[0]
        tris[nf - k: nf - k // 2] = tris[: k - k // 2]                   # duplicates: equal t, the lower index wins
        p = o + 0.25 * d                                                  # a point on ray 0
        tris[1, 0:3] = p                                                  # ray 0 through vertex 0 of face 1 (u = v = 0)
        tris[2, 0:3], tris[2, 3:6] = p + [0, -3, 0], p + [0, 3, 0]        # ray 0 through the edge v0-v1 of face 2
        tris[3] = np.concatenate([o, o + d, o + [0, 0, 5.0]])             # contains the ray: parallel, a = 0
        q = o + 1e-8 * d
        tris[4] = np.concatenate([q + [0, -1, -1], q + [0, 1, -1], q + [0, 0, 1]])          # t around 1e-8
        tris[5] = np.concatenate([q * 1.0000001 + [0, -1, -1], q + [0, 1, -1], q + [0, 0, 1]])
        tris[6, 4] = np.nan                                               # NaN corner
    return cc, ca, tris


@pytest.mark.parametrize("nf,n_aorta,n_cor", [(1, 3, 4), (255, 17, 16), (256, 16, 16), (257, 5, 60), (700, 17, 16),
                                              (1300, 9, 30)])
def test_occlusion_random_matches_checker(engine, nf, n_aorta, n_cor):
    cc, ca, tris = _random_scene(nf * 7 + n_cor, nf, n_aorta, n_cor)
    pts = np.concatenate([tris.reshape(-1, 3)[::5], np.random.default_rng(nf).uniform(-5, 20, (300, 3))])
    pts[3] = np.nan
    want_rm, want_ex = LC.occluded(cc, ca, 1e9, pts, tris, 1.0)
    got_rm, got_ex = _device_occlusion(engine, cc, ca, 1e9, pts, tris, 1.0)
    assert got_ex == want_ex
    assert np.array_equal(got_rm, want_rm)
    if nf >= 255:
        assert want_ex                                       # the >= 3 rule fired


def test_occlusion_duplicate_faces_keep_the_lower_index(engine):
    plane = lambda xx: [xx, -5, -5, xx, 5, -5, xx, 0, 5]
    tris = np.array([plane(8.0), plane(3.0), plane(5.0), plane(3.0), plane(3.0)])
    cc, ca = np.array([[10.0, 0.0, 0.0]]), np.array([[0.0, 0.0, 0.0]])
    got_rm, got_ex = _device_occlusion(engine, cc, ca, 100.0, [(3.0, 0.0, 0.0)], tris)
    assert got_ex == {1} == LC.occluded(cc, ca, 100.0, [(3.0, 0.0, 0.0)], tris)[1]


def test_occlusion_step_and_range_edges(engine):
    cc, ca, tris = _random_scene(3, 300, 4, 40)
    pts = tris.reshape(-1, 3)[::7]
    for rng_mm, step in [(0.0, 1.0), (float("nan"), 1.0), (float("inf"), 3.0), (5.0, 1e300), (-3.0, 1.0)]:
        want_rm, want_ex = LC.occluded(cc, ca, rng_mm, pts, tris, step)
        got_rm, got_ex = _device_occlusion(engine, cc, ca, rng_mm, pts, tris, step)
        assert got_ex == want_ex and np.array_equal(got_rm, want_rm), (rng_mm, step)
    with pytest.raises(RuntimeError):                       # step 0 (step_by(0) panics in the reference)
        _device_occlusion(engine, cc, ca, 10.0, pts, tris, 0.0)
    # empty points, faces or aortic centerline: nothing removed, even with a step of 0
    assert not _device_occlusion(engine, cc, ca, 10.0, np.zeros((0, 3)), tris, 0.0)[0].any()
    assert not _device_occlusion(engine, cc, ca, 10.0, pts, np.zeros((0, 9)), 0.0)[0].any()
    assert not _device_occlusion(engine, cc, np.zeros((0, 3)), 10.0, pts, tris, 0.0)[0].any()


def test_occlusion_acute_takeoff_excludes_the_aortic_wall(engine):
    v, f, ca, cr, _, n_aorta_faces = mm.synth.synthetic_takeoff_mesh(acute_takeoff=True)
    found = v[LC.bounded(cr, v, 3.0)]
    sel = LC.faces_near(v, f, found)
    tris = v[f[sel]].reshape(-1, 9)
    want_rm, want_ex = LC.occluded(cr, ca, 60.0, found, tris, 1.0)
    got_rm, got_ex = _device_occlusion(engine, cr, ca, 60.0, found, tris, 1.0)
    assert got_ex == want_ex and np.array_equal(got_rm, want_rm)
    face_ids = np.nonzero(sel)[0][sorted(got_ex)]
    assert len(face_ids) > 0 and (face_ids < n_aorta_faces).all()   # the aortic wall in front of the coronary
    assert got_rm.any() and not got_rm.all()
    kept = mm.remove_occluded_points_ray_triangle(_cl(cr), _cl(ca), 60.0, found, tris.reshape(-1, 3, 3), 1.0,
                                                  engine=engine)
    assert np.array_equal(kept, found[~want_rm])


def test_occlusion_control_without_three_hits_removes_nothing(engine):
    v, f, ca, cr, _, n_aorta_faces = mm.synth.synthetic_takeoff_mesh(acute_takeoff=True)
    found = v[LC.bounded(cr, v, 3.0)]
    tris = v[f[:n_aorta_faces]].reshape(-1, 9)            # the aortic wall alone: every ray crosses it once
    want_rm, want_ex = LC.occluded(cr, ca, 60.0, found, tris, 1.0)
    got_rm, got_ex = _device_occlusion(engine, cr, ca, 60.0, found, tris, 1.0)
    assert got_ex == want_ex == set() and not got_rm.any() and not want_rm.any()


def test_bounded_points_exact_radius_and_known_answers(engine):
    cl = _cl([(0.0, 0.0, 0.0), (0.0, 0.0, 10.0)])
    pts = np.array([(3.0, 0.0, 0.0), (np.nextafter(3.0, 4.0), 0.0, 0.0), (0.0, 3.0, 10.0), (0.0, 0.0, 5.0),
                    (3.0, 0.0, 0.0), (np.nan, 0.0, 0.0)])
    got = mm.find_centerline_bounded_points_simple(cl, pts, 3.0, engine=engine)
    assert np.array_equal(got, pts[LC.bounded(cl.xyz(), pts, 3.0)])
    assert got.tolist() == [[3.0, 0.0, 0.0], [0.0, 3.0, 10.0], [3.0, 0.0, 0.0]]
    inside = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.5, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 1.0), (0.5, 1.0, 1.0),
              (0.0, 0.0, 2.0), (1.0, 0.0, 2.0), (0.5, 1.0, 2.0)]
    outside = [(-1.0, -1.0, 0.5), (2.0, -1.0, 0.5), (0.5, 2.0, 0.5), (-1.0, -1.0, 1.5), (2.0, -1.0, 1.5)]
    got = mm.find_centerline_bounded_points_simple(_cl([(0.5, 0.5, z) for z in (0.0, 1.0, 2.0)]), inside + outside, 1.0,
                                                   engine=engine)
    assert got.tolist() == [list(p) for p in inside]
    with pytest.raises(ValueError):
        mm.find_centerline_bounded_points_simple(cl, np.zeros((0, 3)), 3.0, engine=engine)
    with pytest.raises(ValueError):
        mm.find_centerline_bounded_points_simple(_cl(np.zeros((0, 3))), pts, 3.0, engine=engine)
    big = np.random.default_rng(5).uniform(-20, 20, (20000, 3))
    clb = np.random.default_rng(6).uniform(-20, 20, (700, 3))
    got = mm.find_centerline_bounded_points_simple(_cl(clb), big, 2.5, engine=engine)
    assert np.array_equal(got, big[LC.bounded(clb, big, 2.5)])


def test_faces_near_points_exact_tol_and_known_answers(engine):
    grid_v = [(float(x), float(y), 0.0) for y in range(3) for x in range(3)]
    grid_f = [[0, 1, 3], [1, 4, 3], [1, 2, 4], [2, 5, 4], [3, 4, 6], [4, 7, 6], [4, 5, 7], [5, 8, 7]]
    got = mm.find_faces_near_points(grid_v, grid_f, [(0.0, 0.0, 0.0)], engine=engine)
    assert got.tolist() == [[list(grid_v[0]), list(grid_v[1]), list(grid_v[3])]]
    assert mm.find_faces_near_points(grid_v, grid_f, [(1.0, 1.0, 0.0)], engine=engine).shape == (6, 3, 3)
    assert mm.find_faces_near_points(grid_v, grid_f, np.zeros((0, 3)), engine=engine).shape == (0, 3, 3)
    assert mm.find_faces_near_points(grid_v, grid_f, [(99.0, 99.0, 0.0)], engine=engine).shape == (0, 3, 3)
    got = mm.find_faces_near_points(grid_v, grid_f, [(0.5, 0.0, 0.0)], tol=0.5, engine=engine)   # exactly tol away
    assert got.shape[0] == int(LC.faces_near(grid_v, grid_f, [(0.5, 0.0, 0.0)], 0.5).sum()) == 3
    with pytest.raises(RuntimeError):
        mm.find_faces_near_points(grid_v, grid_f + [[0, 1, 9]], [(0.0, 0.0, 0.0)], engine=engine)
    v, f, *_ = mm.synth.synthetic_takeoff_mesh()
    pts = v[::3]
    sel = LC.faces_near(v, f, pts)
    assert np.array_equal(mm.find_faces_near_points(v, f, pts, engine=engine), v[f[sel]])


@pytest.mark.parametrize("acute", [True, False])
def test_label_geometry_end_to_end(engine, acute):
    v, f, ca, cr, cl, _ = mm.synth.synthetic_takeoff_mesh(acute_takeoff=acute)
    res = mm.label_geometry((v, f), _cl(ca), _cl(cr), _cl(cl), acute_takeoff_rca=acute, control_plot=False,
                            engine=engine)
    lab = LC.label_geometry(v, f, ca, cr, cl, acute_rca=acute)
    keys = ["aorta_points", "rca_points", "lca_points", "rca_removed_points", "lca_removed_points"]
    assert set(res) == {"mesh"} | set(keys)
    for k, key in enumerate(keys):
        assert np.array_equal(res[key], v[lab == k]), key
    assert (res["rca_removed_points"].shape[0] > 0) == acute
    assert res["rca_points"].shape[0] > 0 and res["lca_points"].shape[0] > 0

    class Mesh:                                             # anything with .vertices / .faces
        vertices, faces = v, f
    m = Mesh()
    res2 = mm.label_geometry(m, _cl(ca), _cl(cr), _cl(cl), acute_takeoff_rca=acute, engine=engine)
    assert res2["mesh"] is m and all(np.array_equal(res2[k], res[k]) for k in keys)
    # the dict feeds the existing consumers
    frames = _cl(cr).xyz()[10:30:2]
    prox, dist, betw = mm.find_points_by_cl_region(_cl(cr), frames, res["rca_points"], engine=engine)
    assert prox.shape[0] + dist.shape[0] + betw.shape[0] == res["rca_points"].shape[0]
