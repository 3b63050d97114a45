"""Rim conditioning on the device (csrc/mm_rim_kernels.hip, csrc/mm_rim.cpp) against the checker
(tests/mm_checkers/rim_condition.py).  Indices, counts and flags are exact; coordinates the three mesh-wide stages
produce from the same inputs are bit-identical; coordinates that pass through the plane fit differ from numpy's SVD by
rounding and are compared at 1e-9 mm (tests/test_rim_host.py derives the bound).  The conditions under which that
holds are asserted on the checker's own intermediates.  Shapes are the smallest at which each kernel can go wrong."""
import numpy as np
import pytest

from mm_checkers import rim_condition as K
from mm_checkers import stitch_mesh as SK
from test_trim_host import octahedron, capped_tube
from test_stitch_host import edge_counts, same_bits
from test_gpu_stitch import takeoff_case
from test_rim_host import HAND_CASES, TOL, irregular_ring

import multimoda_rs_amd as mm

pytestmark = pytest.mark.gpu
ccta = mm.ccta
CHUNK = 1024                                                            # mm_rim_locate_chunk_points()


# ---- locate --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nv", [1, 255, 256, 257])
@pytest.mark.parametrize("r", [1, 64, CHUNK + 1])
def test_locate(engine, nv, r):
    assert mm._native.lib().mm_rim_locate_chunk_points() == CHUNK
    rng = np.random.default_rng(1000 * nv + r)
    v = np.round(rng.normal(size=(nv, 3)), 1)                           # a coarse grid: duplicates, the last one wins
    if nv >= 3:
        v[1] = [np.nan, 0.5, 0.5]
        v[nv - 1] = v[0]
    v[nv // 2] = [-0.0, 0.0, 1.5]
    pts = v[rng.integers(0, nv, r)].copy()
    pts[pts == 0.0] = -0.0                                              # -0.0 against 0.0
    pts[::7] += 100.0                                                   # absent
    if r > 1:
        pts[-1] = [np.nan, 0.5, 0.5]                                    # a NaN row equals nothing, not even itself
        pts[1] = [0.0, -0.0, 1.5]
    got, want = ccta.locate_points(v, pts, engine), K.locate_points(v, pts)
    assert np.array_equal(got, want)
    assert want[0] == -1 and (r == 1 or (want[-1] == -1 and want[1] >= 0))
    if nv >= 3 and r == 64:
        assert ccta.locate_points(v, v[:1], engine)[0] == nv - 1


def test_locate_empty(engine):
    assert ccta.locate_points(np.zeros((0, 3)), [[1.0, 2, 3]], engine).tolist() == [-1]
    assert ccta.locate_points([[1.0, 2, 3]], np.zeros((0, 3)), engine).shape == (0,)


# ---- layers and push ------------------------------------------------------------------------------------------------------

def tube_case():
    v, f = capped_tube(12, 9)
    r = np.random.default_rng(5)
    v = v + np.concatenate([0.01 * r.normal(size=(len(v) - 2, 3)), np.zeros((2, 3))])      # the cap centres stay on the axis
    v = np.concatenate([v, [[9.0, 9.0, 9.0]]])                          # an unreferenced vertex
    f = np.concatenate([f, [[5, 5, 17]]])                               # a degenerate face with a repeated index
    return v, f


LAYER_CASES = {
    # name: (mesh, seeds, n_rings, expected rings run)
    "ring_seeds_1": (tube_case(), list(range(12)), 1, 1),
    "ring_seeds_2": (tube_case(), list(range(12)), 2, 2),
    "ring_seeds_5": (tube_case(), list(range(12)), 5, 5),
    "isolated_seed": (tube_case(), [110], 2, 1),
    "empty_seeds": (tube_case(), [], 2, 0),
    "frontier_dies": (octahedron(), [4], 5, 3),
    "one_face": ((octahedron()[0], octahedron()[1][:1]), [0], 2, 2),
    "faces_257": ((capped_tube(16, 9)[0], capped_tube(16, 9)[1][:257]), [3, 40], 2, 2),
}


@pytest.mark.parametrize("name", sorted(LAYER_CASES))
def test_layers_and_push(engine, name):
    (v, f), seeds, n_rings, rings_want = LAYER_CASES[name]
    origin, normal, step = np.array([0.0, 0.0, 0.3]), np.array([0.0, 0.0, 1.0]), 0.1
    (wv, _), wl, rings_run, r_norms = K.enforce_layer_gap_from_plane((v, f), seeds, origin, normal, step, n_rings)
    assert rings_run == rings_want
    assert not any(1e-11 <= rn <= 1e-9 for rn in r_norms)               # none within a factor 10 of the 1e-10 threshold
    (gv, gf), gl, info = ccta.enforce_layer_gap_from_plane((v, f), seeds, origin, normal, step, n_rings, engine=engine,
                                                           return_info=True)
    assert np.array_equal(gl, wl) and gl.dtype == np.int32
    assert same_bits(gv, wv) and np.array_equal(gf, f)
    pushed = int((wl >= 1).sum())
    assert info["rings_run"] == rings_run and info["n_layer_vertices"] == pushed
    assert info["launches"] == (0 if not seeds else 1 + rings_run + (1 if pushed else 0))
    if name.startswith("ring_seeds"):
        assert set(wl[12:24]) == {1} and wl[108] == 1                   # the cap centre: on the axis, layer 1, skipped
        assert 0.0 in r_norms and same_bits(gv[108], v[108])
        assert (n_rings == 1) == (wl[24] == -1)                         # reachable over rings 1 and 2: ring 1 claims first
        assert wl[110] == -1
        assert not same_bits(gv[12:24], v[12:24])
    if name == "frontier_dies":
        assert wl.tolist() == [1, 1, 1, 1, 0, 2] and info["launches"] == 5      # below the 1 + 5 + 1 of n_rings = 5


# ---- split -----------------------------------------------------------------------------------------------------------------

def check_split(engine, mesh, ring, counts, **caps):
    (wv, wf), wdense, winfo = K.split_rim_edges(mesh, ring, counts)
    gv, gf, gdense, ginfo = ccta.split_rim_edges(mesh[0], mesh[1], ring, counts, engine, **caps)
    assert np.array_equal(gf, wf) and gdense.tolist() == wdense
    assert same_bits(gv, wv)
    for k, x in winfo.items():
        assert ginfo[k] == x, k
    touched = winfo["n_fanned_faces"]
    assert ginfo["launches"] == (3 if len(mesh[1]) else 2) + (4 if touched else 0)
    return gv, gf, gdense, ginfo


@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_split_hand_meshes(engine, name):
    mesh, ring, counts = HAND_CASES[name]
    check_split(engine, mesh, ring, counts)


def open_tube(n_around, n_rings=4, seed=3):
    c = np.stack([np.zeros(n_rings), np.zeros(n_rings), np.arange(n_rings, dtype=float)], 1)
    v, f = mm.synth._tube(c, np.tile([1.0, 0, 0], (n_rings, 1)), np.tile([0, 1.0, 0], (n_rings, 1)), 2.0, n_around)
    r = np.random.default_rng(seed)
    return v + 0.05 * r.normal(size=v.shape), f


@pytest.mark.parametrize("target", [17, 32, 100])
@pytest.mark.parametrize("reverse", [False, True])
def test_split_tube_end(engine, target, reverse):
    v, f = open_tube(16)
    idx = list(range(16))
    if reverse:
        idx = idx[:1] + idx[:0:-1]
    counts, status, gap = K.densify_plan(v[idx], target)
    assert status == 1 and gap >= 1e-6
    before = edge_counts(f)
    gv, gf, dense, info = check_split(engine, (v, f), idx, counts)
    assert len(dense) == target and info["n_inserted"] == target - 16
    # the open edge of the result at this end is one ring of exactly target vertices: the returned ring, no T-junction
    rings = mm.order_boundary_rings(gf, gv, seeds={int(dense[0])}, engine=engine)
    assert len(rings) == 1 and len(rings[0]) == target and set(rings[0].tolist()) == set(dense.tolist())
    assert max(edge_counts(gf).values()) <= max(before.values()) == 2
    # densify_boundary from the coordinates gives the same mesh
    mesh2, dense_pts, dinfo = ccta.densify_boundary((v, f), v[idx], target, engine=engine)
    assert same_bits(mesh2[0], gv) and np.array_equal(mesh2[1], gf) and same_bits(dense_pts, gv[dense])


@pytest.mark.parametrize("nf", [1, 256, 257])
def test_split_face_counts_and_triangle_ring(engine, nf):
    v, f = open_tube(16, 10)
    assert len(f) >= 257
    counts = [2, 0, 1] + [0] * 12 + [3]
    check_split(engine, (v, f[:nf]), list(range(16)), counts)
    tv, tf = open_tube(3)                                               # n = 3: every pair of ring vertices is a ring edge
    check_split(engine, (tv, tf), [0, 1, 2], [1, 0, 2])
    check_split(engine, (tv, tf), [0, 2, 1], [1, 1, 1])


def test_split_capacity_retry_and_rejections(engine):
    v, f = open_tube(16)
    counts = [1] * 16
    _, _, _, info = check_split(engine, (v, f), list(range(16)), counts, vert_cap=len(v), face_cap=len(f))
    assert info["attempts"] == 2 and info["n_vertices"] == len(v) + 16 and info["n_faces"] == len(f) + 16
    _, _, _, info = check_split(engine, (v, f), list(range(16)), counts)
    assert info["attempts"] == 1
    with pytest.raises(ValueError, match="twice"):
        ccta.split_rim_edges(v, f, [0, 1, 2, 1], [1, 0, 0, 0], engine)
    with pytest.raises(ValueError, match="out of range"):
        ccta.split_rim_edges(v, f, [0, 1, len(v)], [1, 0, 0], engine)
    with pytest.raises(ValueError, match="different targets"):
        ccta.write_ring_to_mesh((v, f), [v[0], v[0]], [[1.0, 2, 3], [1.0, 2, 4]], engine=engine)
    mesh2, moved = ccta.write_ring_to_mesh((v, f), v[[3, 5]], [[1.0, 2, 3], [4.0, 5, 6]], engine=engine)
    assert moved == [3, 5] and mesh2[0][5].tolist() == [4.0, 5.0, 6.0] and same_bits(mesh2[0][6:], v[6:])


# ---- the whole stage ---------------------------------------------------------------------------------------------------------

REPORT_EXACT = ("n_vertices", "n_faces", "n_moved_prox", "n_moved_dist", "n_moved_ostium", "clamped", "n_layer_vertices",
                "n_inserted_prox", "n_inserted_dist", "n_fanned_faces", "n_centroid_fans", "ring_over_target", "ring_off_mesh")


def expected_launches(rep):
    """The count include/mm_ccta.h documents, from what the report says happened."""
    n = 2 * 2                                                           # both rings located and written
    if rep["plane_angle_deg"] > 0.0 or rep["n_moved_ostium"]:
        n += 2                                                          # the ostium stage's write-back
        if rep["clamped"] and rep["n_moved_ostium"]:
            l1, l2 = rep["n_layer_vertices"]
            n += 1 + (1 if l1 == 0 else 2) + (1 if l1 + l2 else 0)
    for s, key in enumerate(("n_inserted_prox", "n_inserted_dist")):
        if rep[key]:
            n += 1 + 3 + 4                                              # located, split, compacted (every rim edge has an owner)
        elif rep["ring_off_mesh"][s]:
            n += 1
    return n


def check_conditions(wrep, threshold=45.0):
    assert all(g >= 0.1 for g in wrep["gaps"]), wrep["gaps"]
    assert all(g >= 1e-6 for g in wrep["plan_gaps"]), wrep["plan_gaps"]
    if wrep["plane_angle_deg"]:
        assert abs(wrep["plane_angle_deg"] - threshold) >= 5.0
    if wrep["worst_plus_overshoot"] is not None:
        assert abs(wrep["worst_plus_overshoot"]) >= 1e-3
    assert not any(1e-11 <= rn <= 1e-9 for rn in wrep["r_norms"])


def check_whole_stage(engine, mesh, results, geom, frames, **kw):
    got = mm.condition_boundary_rings(mesh, results, geom, engine=engine, **kw)
    n_iv = kw.get("n_points_iv_cont", 100)
    first = SK.downsample(frames[0], n_iv)
    rings = [results["boundary_points_1"], results["boundary_points_2"]]
    i, j, _ = SK.assign_rings_to_ends(rings, geom.centroids[0], geom.centroids[-1])
    target = max(3, round(kw.get("boundary_point_ratio", 1.0) * len(first)))
    wp, wd, (wv, wf), wrep = K.prepare_prox_dist_boundary_pts(
        mesh, rings[i], rings[j], geom.centroids[0], proximal_is_ostium=kw.get("proximal_is_ostium", True),
        proximal_iv_frame_pts=first, clamp_overshoot=kw.get("clamp_overshoot", 0.5), target_n=target,
        prox_outward=geom.centroids[0] - geom.centroids[-1], aorta_pts=results.get("aorta_points"))
    check_conditions(wrep)
    gv, gf = got["mesh"]
    rep = got["rim_report"]
    assert np.array_equal(gf, wf)
    assert gv.shape == wv.shape and np.abs(gv - wv).max() < TOL
    assert np.abs(got["boundary_points_1"] - wp).max() < TOL and np.abs(got["boundary_points_2"] - wd).max() < TOL
    assert same_bits(got["boundary_points"], np.concatenate([got["boundary_points_1"], got["boundary_points_2"]]))
    for k in REPORT_EXACT:
        assert rep[k] == wrep[k], (k, rep[k], wrep[k])
    assert abs(rep["plane_shift_mm"] - wrep["plane_shift_mm"]) < TOL and abs(rep["plane_angle_deg"] - wrep["plane_angle_deg"]) < 1e-9
    assert rep["target_n"] == target and rep["n_prox"] == len(wp) and rep["n_dist"] == len(wd)
    # structure: the mesh goes up once and comes down once, everything else is ring-sized; the documented launches
    v0, f0 = mm.ccta._mesh_parts(mesh)
    ring_bytes = 64 * max(target, len(rings[i]), len(rings[j]))
    assert rep["n_launches"] == expected_launches(rep)
    assert len(v0) * 24 + len(f0) * 12 <= rep["bytes_uploaded"] <= len(v0) * 24 + len(f0) * 12 + 40 * ring_bytes
    assert len(gv) * 24 + len(gf) * 12 <= rep["bytes_downloaded"] <= len(gv) * 24 + len(gf) * 12 + 40 * ring_bytes
    # the rings are the mesh's real open edge
    idx = K.locate_points(gv, got["boundary_points_1"])
    assert (idx >= 0).all()
    return got, wrep


@pytest.fixture(scope="module")
def takeoff(engine):
    res, geom, frames = takeoff_case(engine)
    cut = mm.remove_labeled_points_from_mesh(dict(res), "section_points", target_boundaries=2, engine=engine)
    assert "boundary_points_2" in cut
    return res, cut, geom, frames


@pytest.mark.parametrize("ostium", [True, False])
@pytest.mark.parametrize("ratio", [1.0, 0.5])
def test_whole_stage_on_the_takeoff_mesh(engine, takeoff, ostium, ratio):
    _, cut, geom, frames = takeoff
    got, wrep = check_whole_stage(engine, cut["mesh"], cut, geom, frames, proximal_is_ostium=ostium, boundary_point_ratio=ratio)
    rep = got["rim_report"]
    assert rep["n_prox"] == rep["n_dist"] == rep["target_n"] == (32 if ratio == 1.0 else 16)
    assert rep["attempts"] == 1 and rep["n_leftover_rings"] == 0
    if not ostium:
        assert rep["plane_angle_deg"] == 0.0 and rep["clamped"] == 0


def tilted_case():
    """An open tube whose proximal rim plane cuts a steeply tilted first IV frame: the plane shift and the clamp fire."""
    v, f = open_tube(16, 7, seed=9)
    frames = []
    t = np.linspace(0, 2 * np.pi, 32, endpoint=False)
    r = np.random.default_rng(4)
    for k, z in enumerate((-0.2, 2.0, 4.0, 6.2)):
        ang = np.radians(62.0) if k == 0 else 0.0
        ring = np.stack([1.5 * np.cos(t), 1.5 * np.sin(t) * np.cos(ang), 1.5 * np.sin(t) * np.sin(ang) + z], 1)
        frames.append(ring + 0.01 * r.normal(size=ring.shape))
    results = {"boundary_points_1": v[:16], "boundary_points_2": v[-16:], "mesh": (v, f),
               "aorta_points": np.array([[0.3, 0.2, 9.0], [-0.2, 0.1, 11.0], [0.1, -0.4, 10.0]])}
    return (v, f), results, mm.FlatGeometry.from_frames(frames), frames


def test_whole_stage_shift_and_clamp(engine):
    mesh, results, geom, frames = tilted_case()
    got, wrep = check_whole_stage(engine, mesh, results, geom, frames)
    rep = got["rim_report"]
    assert rep["clamped"] == 1 and rep["plane_shift_mm"] > 0 and rep["n_moved_ostium"] == 16
    assert rep["n_layer_vertices"] == [16, 16]


def test_capacity_retry_of_the_whole_stage(engine):
    mesh, results, geom, frames = tilted_case()
    v, f = mesh
    args = (v, f, results["boundary_points_1"], results["boundary_points_2"], frames[0], geom.centroids[0],
            geom.centroids[0] - geom.centroids[-1], results["aorta_points"],
            {"proximal_is_ostium": True, "target_n": 32, "angle_threshold_deg": 45.0, "clamp_overshoot": 0.5}, engine)
    gv, gf, gp, gd, rep = ccta._condition(*args, vert_cap=len(v), face_cap=len(f))
    wv, wf, wp, wd, wrep = ccta._condition(*args)
    assert rep["attempts"] >= 2 and wrep["attempts"] == 1
    assert same_bits(gv, wv) and np.array_equal(gf, wf) and same_bits(gp, wp) and same_bits(gd, wd)
    assert rep["n_vertices"] == len(v) + 32 and rep["n_faces"] == len(f) + 32


# ---- the line ----------------------------------------------------------------------------------------------------------------

def test_stitch_conditioned(engine, takeoff):
    res, cut, geom, frames = takeoff
    got = mm.stitch_conditioned(dict(res), geom, region_remove="section_points", engine=engine)
    cond = mm.condition_boundary_rings(cut["mesh"], cut, geom, engine=engine)
    want = mm.stitch_ccta_to_intravascular(geom, cond["mesh"], cond, prox_start_mode="highest_z", engine=engine)
    gv, gf = got["mesh"]
    assert same_bits(gv, want["mesh"][0]) and np.array_equal(gf, want["mesh"][1])
    assert got["rim_report"] == cond["rim_report"] and got["stitch_report"] == want["stitch_report"]
    n_iv = len(frames[0])
    prox_b, dist_b = got["prox_boundary_points"], got["dist_boundary_points"]
    assert len(prox_b) == len(dist_b) == n_iv == 32                     # the strips are 1 : 1
    assert got["stitch_report"]["n_nonmanifold_edges"] == 0
    counts = edge_counts(gf)
    for b in (prox_b, dist_b):
        idx = set(mm.ccta._match(gv, b).tolist())
        assert -1 not in idx and len(idx) == n_iv
        for e, c in counts.items():
            if e & idx:
                assert c == 2, (sorted(e), c)
    # the unconditioned line is what it was
    plain = mm.stitch(dict(res), geom, region_remove="section_points", engine=engine)
    old = mm.stitch_ccta_to_intravascular(geom, cut["mesh"], cut, prox_start_mode="highest_z", engine=engine)
    assert same_bits(plain["mesh"][0], old["mesh"][0]) and np.array_equal(plain["mesh"][1], old["mesh"][1])
    assert "rim_report" not in plain and len(plain["prox_boundary_points"]) == 16
    filled = mm.stitch_conditioned(dict(res), geom, region_remove="section_points", fill_holes=True, engine=engine)
    assert "fill_report" in filled and "rim_report" in filled
