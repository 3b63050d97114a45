"""CCTA mesh closing on the device (csrc/mm_close_kernels.hip, csrc/mm_close.cpp) against the checker
(tests/mm_checkers/close_mesh.py): identical indices, bit-identical coordinates and volume.  Hole filling on the box, the
capped tube without one and both caps, the octahedron without every subset of faces, two bodies, an inside-out body, a
pinch and a non-manifold fin, randomly reversed faces with and without the winding stage, and the capacity retry; the
line label -> remove -> stitch(fill_holes=True) on the synthetic take-off mesh; the label smoothing in both forms; the
wall mesh; launch counts from the reports."""
import itertools
import math

import numpy as np
import pytest

from mm_checkers import close_mesh as CM
from mm_checkers import trim_mesh as TM
from test_trim_host import octahedron, capped_tube
from test_stitch_host import same_bits
from test_close_host import open_box, two_bodies, pinched
from test_gpu_stitch import cl_of, takeoff_case, messy_mesh

import multimoda_rs_amd as mm
from multimoda_rs_amd import ccta

pytestmark = pytest.mark.gpu

FILL_KEYS = ("n_vertices", "n_faces", "n_loops_filled", "n_fan_faces", "n_open_edges_before", "n_short_loops",
             "n_irregular_components", "n_irregular_edges", "n_open_edges", "n_nonmanifold_edges", "n_flipped_faces",
             "inverted", "watertight")


def round_bound(nf):
    return 2 + math.ceil(math.log2(max(nf, 2)))


def bits_equal(a, b):
    return np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


def canon(faces):
    """The oriented triangles as a set: every face rotated so that its smallest index leads."""
    return {tuple(np.roll(t, -int(np.argmin(t)))) for t in np.asarray(faces).tolist()}


def same_fill(v, f, engine, fix=True):
    gv, gf, gr = mm.fill_holes(v, f, fix, engine=engine)
    wv, wf, wr = CM.fill_holes(v, f, fix)
    assert same_bits(gv, wv)
    assert np.array_equal(gf, wf) and gf.dtype == np.int64
    for k in FILL_KEYS:
        assert gr[k] == wr[k], (k, gr[k], wr[k])
    assert bits_equal(gr["volume"], wr["volume"]), (gr["volume"], wr["volume"])
    nf = len(np.asarray(f).reshape(-1, 3))
    assert (gr["winding_rounds"] == 0) if (not fix or nf == 0) else (1 < gr["winding_rounds"] <= round_bound(nf))
    if wr["n_irregular_components"] == 0 and wr["n_nonmanifold_edges"] == 0 and wr["n_short_loops"] == 0:
        assert gr["n_open_edges"] == 0 and gr["watertight"]
    return gv, gf, gr


# ---- hole filling ---------------------------------------------------------------------------------------------------------

def test_box(engine):
    v, f = open_box()
    gv, gf, rep = same_fill(v, f, engine)
    assert len(gf) == 14 and gv[8].tolist() == [0.5, 0.5, 1.0] and rep["n_loops_filled"] == 1 and rep["volume"] == 1.0
    m = mm.manual_hole_fill((v, f), engine=engine)
    assert same_bits(m[0], gv) and np.array_equal(m[1], gf)

    class Mesh:
        def __init__(self, vertices, faces):
            self.vertices, self.faces = vertices, faces

    src = Mesh(v, f)
    m = mm.manual_hole_fill(src, engine=engine)
    assert isinstance(m, Mesh) and m is not src and np.array_equal(m.faces, gf) and len(src.faces) == 10


def test_capped_tube_without_caps(engine):
    v, f = capped_tube(12, 9)
    assert same_fill(v, f, engine)[2]["n_loops_filled"] == 0                 # closed: nothing to do
    assert same_fill(v, f[:-12], engine)[2]["n_loops_filled"] == 1
    gv, gf, rep = same_fill(v, f[:-24], engine)
    assert rep["n_loops_filled"] == 2 and rep["n_fan_faces"] == 24 and rep["watertight"]
    same_fill(v, f[:-24], engine, fix=False)


def test_octahedron_every_subset_of_faces_removed(engine):
    v, f = octahedron()
    regular = 0
    for bits in itertools.product([False, True], repeat=len(f)):
        keep = ~np.array(bits)
        if not keep.any():
            continue
        _, _, rep = same_fill(v, f[keep], engine)
        regular += rep["n_irregular_components"] == 0 and rep["n_loops_filled"] > 0
    assert regular >= 8                                                   # every single face removed, at the least


def test_two_bodies_and_inside_out(engine):
    v, f = two_bodies()
    _, _, rep = same_fill(v, f, engine)                                   # the tube is wound inwards and outweighs the box
    assert rep["n_loops_filled"] == 2 and rep["inverted"] == 1 and rep["volume"] < 0 and rep["watertight"]
    _, gf, rep = same_fill(v, f[:, ::-1], engine)
    assert rep["inverted"] == 0 and rep["volume"] > 0 and rep["watertight"]
    bv, bf = open_box()
    _, gf, rep = same_fill(bv, bf[:, ::-1], engine)
    assert rep["inverted"] == 1 and canon(gf) == canon(CM.fill_holes(bv, bf)[1])      # the walk ran the other way round


def test_pinch_and_fin(engine):
    v, f = pinched()
    for fix in (True, False):
        _, _, rep = same_fill(v, f, engine, fix)
        assert rep["n_irregular_components"] == 1 and rep["n_irregular_edges"] == 8 and rep["n_loops_filled"] == 1
        assert rep["n_open_edges"] == 8
    bv, bf = open_box()                                                   # a fin on the bottom edge 0 - 1
    fv = np.concatenate([bv, [[0.5, -1.0, -1.0]]])
    ff = np.concatenate([bf, [[0, 1, 8]]])
    _, _, rep = same_fill(fv, ff, engine)
    assert rep["n_nonmanifold_edges"] == 1 and rep["n_loops_filled"] >= 1
    same_fill(fv, ff, engine, fix=False)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_randomly_reversed_faces(engine, seed):
    v, f = capped_tube(16, 12)
    f = f[:-32]
    r = np.random.default_rng(seed)
    g = f.copy()
    m = r.random(len(g)) < 0.3
    g[m] = g[m][:, ::-1]
    _, gf, rep = same_fill(v, g, engine, fix=True)
    _, pf, prep = same_fill(v, f, engine, fix=True)
    assert rep["watertight"] and rep["n_loops_filled"] == 2
    # the same surface as from the unreversed input: the same faces up to the rules (face 0 keeps its order, the
    # inversion has the last word), so the same oriented triangles
    assert canon(gf) == canon(pf)
    _, _, rep = same_fill(v, g, engine, fix=False)
    assert rep["n_irregular_components"] == CM.fill_holes(v, g, False)[2]["n_irregular_components"]


def test_messy_mesh_and_empty(engine):
    v, f = messy_mesh(3, nv=3000, nf=8000)
    # short loops, hundreds of irregular components, thousands of non-manifold edges; without the winding stage, whose
    # flips on this mesh's non-orientable components are unspecified
    _, _, rep = same_fill(v, f, engine, False)
    assert rep["n_short_loops"] > 0 and rep["n_irregular_components"] > 100 and rep["n_loops_filled"] > 0
    gv, gf, rep = mm.fill_holes(np.zeros((3, 3)), np.zeros((0, 3), dtype=np.int64), engine=engine)
    assert gv.shape == (3, 3) and gf.shape == (0, 3) and rep["n_faces"] == 0 and rep["watertight"]
    with pytest.raises(ValueError, match="out of range"):
        mm.fill_holes(np.zeros((3, 3)), [[0, 1, 3]], engine=engine)


def test_capacity_retry(engine):
    """A rim longer than the first guess (1024 fan faces, 16 loops): the wrapper retries once with the exact sizes; the C
    call with a short capacity writes the report only."""
    v, f = capped_tube(1500, 3)
    f = f[:-3000]
    _, gf, rep = same_fill(v, f, engine)
    assert rep["n_fan_faces"] == 3000 and len(gf) == len(f) + 3000
    sheets_v, sheets_f = [], []
    for k in range(20):                                                   # 20 open boxes: 20 loops > 16
        bv, bf = open_box()
        sheets_f.append(bf + 8 * k)
        sheets_v.append(bv + [3.0 * k, 0, 0])
    _, _, rep = same_fill(np.concatenate(sheets_v), np.concatenate(sheets_f), engine)
    assert rep["n_loops_filled"] == 20
    N = mm._native
    bv, bf = open_box()
    out_v, out_f = np.full((8, 3), 7.0), np.full((10, 3), 7, dtype=np.int64)
    r = N.MMFillReport()
    import ctypes as C
    rc = N.lib().mm_fill_holes(engine.handle, N._ptr(bv), 8, N._ptr(np.ascontiguousarray(bf, dtype=np.int64)), 10, 1, 8, 10,
                               N._ptr(out_v), N._ptr(out_f), C.byref(r))
    assert rc == -3 and (r.n_vertices, r.n_faces, r.n_loops_filled, r.n_fan_faces) == (9, 14, 1, 4)
    assert (out_v == 7.0).all() and (out_f == 7).all()


# ---- the line label -> remove -> stitch -------------------------------------------------------------------------------

def test_stitch_with_and_without_fill(engine):
    res, geom, frames = takeoff_case(engine)
    plain = mm.stitch(dict(res), geom, region_remove="section_points", engine=engine)
    cut = mm.remove_labeled_points_from_mesh(dict(res), "section_points", target_boundaries=2, engine=engine)
    want = mm.stitch_ccta_to_intravascular(geom, cut["mesh"], cut, prox_start_mode="highest_z", engine=engine)
    assert same_bits(plain["mesh"][0], want["mesh"][0]) and np.array_equal(plain["mesh"][1], want["mesh"][1])
    assert "fill_report" not in plain and plain["stitch_report"] == want["stitch_report"]
    filled = mm.stitch(dict(res), geom, region_remove="section_points", engine=engine, fill_holes=True)
    wv, wf, wr = CM.fill_holes(*want["mesh"])
    assert same_bits(filled["mesh"][0], wv) and np.array_equal(filled["mesh"][1], wf)
    for k in FILL_KEYS:
        assert filled["fill_report"][k] == wr[k], k
    assert bits_equal(filled["fill_report"]["volume"], wr["volume"])
    assert filled["stitch_report"] == want["stitch_report"] and wr["n_loops_filled"] >= 2


# ---- label smoothing ------------------------------------------------------------------------------------------------------

def smooth_both(labels, faces, iterations, engine):
    nv = len(labels)
    rows = CM.adjacency_of_faces(faces, nv)
    want, winfo = CM.smooth_labels(labels, rows, iterations)
    got_f, info_f = ccta.smooth_mesh_labels_info(labels, iterations=iterations, faces=faces, engine=engine)
    got_m, info_m = ccta.smooth_mesh_labels_info(labels, mm.build_adjacency_map(faces), iterations, engine=engine)
    assert got_f.dtype == np.uint8 and np.array_equal(got_f, want) and np.array_equal(got_m, want)
    for info in (info_f, info_m):
        for k in winfo:
            assert info[k] == winfo[k], (k, info, winfo)
    assert info_f["launches"] <= 2 * info_f["iterations_run"] and info_m["launches"] <= info_m["iterations_run"]
    return got_f, info_f


@pytest.mark.parametrize("n_labels", [2, 5, 256])
def test_smoothing_on_the_takeoff_mesh(engine, n_labels):
    v, f, *_ = mm.synth.synthetic_takeoff_mesh(n_theta=48, n_z=30)
    r = np.random.default_rng(n_labels)
    base = (np.arange(len(v)) * n_labels // len(v)).astype(np.uint8)     # bands of one label ...
    noise = r.random(len(v)) < 0.05                                       # ... with a few percent flipped at random
    labels = np.where(noise, r.integers(0, n_labels, len(v)), base).astype(np.uint8)
    for it in (0, 1, 2, 7, 50):
        got, info = smooth_both(labels, f, it, engine)
        assert info["iterations_run"] <= it
    assert info["iterations_run"] < 50 and info["n_flips_last"] == 0       # early stop
    assert info["n_flips"] > 0 or n_labels == 256                           # (bands of 256 labels are too narrow to vote)
    assert np.array_equal(mm.smooth_mesh_labels(labels, mm.build_adjacency_map(f), 7, engine=engine),
                          mm.smooth_mesh_labels(labels, faces=f, iterations=7, engine=engine))
    purely_random = r.integers(0, n_labels, len(v)).astype(np.uint8)
    smooth_both(purely_random, f, 2, engine)


@pytest.mark.parametrize("n_labels", [2, 5, 256])
def test_smoothing_on_random_faces_with_repeated_corners(engine, n_labels):
    r = np.random.default_rng(10 + n_labels)
    nv, nf = 4000, 6000
    f = r.integers(0, nv - 50, (nf, 3))                                   # the last 50 vertices have no face
    f[:300, 1] = f[:300, 0]
    f[300:400, 2] = f[300:400, 0]
    f[400:450] = f[400:450, :1]
    labels = r.integers(0, n_labels, nv).astype(np.uint8)
    for it in (0, 1, 2, 7, 50):
        got, _ = smooth_both(labels, f, it, engine)
        assert np.array_equal(got[-50:], labels[-50:])


def test_smoothing_small_cases_and_errors(engine):
    out, info = ccta.smooth_mesh_labels_info([0, 1, 0, 0], iterations=3, faces=[[0, 1, 2], [1, 2, 3]], engine=engine)
    assert out.tolist() == [0, 0, 0, 0] and info["iterations_run"] == 2 and info["n_flips"] == 1
    assert mm.smooth_mesh_labels([0, 1, 0, 0], {0: {1, 2}, 1: {0, 2, 3}, 2: {0, 1, 3}, 3: {1, 2}}, 3, engine=engine).tolist() == [0] * 4
    for it in range(5):                                                   # the two-vertex swap
        out, info = ccta.smooth_mesh_labels_info([3, 7], {0: [1], 1: [0]}, it, engine=engine)
        assert out.tolist() == ([7, 3] if it % 2 else [3, 7]) and info["n_flips"] == 2 * it
    # asymmetric rows: 0 listens to 1, nobody listens to 0
    assert mm.smooth_mesh_labels([1, 2, 2], {0: [1], 1: [2], 2: [1, 1]}, 1, engine=engine).tolist() == [2, 2, 2]
    assert mm.smooth_mesh_labels([1, 2, 3], {0: [1, 2]}, 5, engine=engine).tolist() == [1, 2, 3]
    with pytest.raises(ValueError, match="exactly one"):
        mm.smooth_mesh_labels([1, 2], engine=engine)
    with pytest.raises(ValueError, match="exactly one"):
        mm.smooth_mesh_labels([1, 2], {0: [1]}, faces=[[0, 1, 1]], engine=engine)
    with pytest.raises(ValueError, match="out of range"):
        mm.smooth_mesh_labels([1, 2], {0: [2]}, engine=engine)
    N = mm._native
    lab, out, info = np.array([1, 2], dtype=np.uint8), np.full(2, 9, dtype=np.uint8), np.zeros(4, dtype=np.int64)
    off, nb = np.array([0, 1, 2], dtype=np.int64), np.array([1, 2], dtype=np.int64)
    rc = N.lib().mm_smooth_labels_csr(engine.handle, N._ptr(lab), 2, N._ptr(off), N._ptr(nb), 1, N._ptr(out), N._ptr(info))
    assert rc == -2 and out.tolist() == [9, 9]


# ---- wall mesh ------------------------------------------------------------------------------------------------------------

def test_wall_mesh(engine):
    v, f, ca, cr, cll, _ = mm.synth.synthetic_takeoff_mesh()
    cla, clr, cl_l = cl_of(ca), cl_of(cr), cl_of(cll)
    res = mm.label_geometry((v, f), cla, clr, cl_l, acute_takeoff_rca=True, engine=engine)
    # the sub-mesh the fill sees is of the kind the no-open-edge property speaks of
    sub = TM.keep_labeled_points_from_mesh(dict(res), ["aorta_points", "rca_removed_points", "lca_removed_points"])
    srep = CM.fill_holes(*sub["mesh"])[2]
    assert srep["n_irregular_components"] == 0 and srep["n_nonmanifold_edges"] == 0 and srep["n_loops_filled"] >= 2
    same_fill(*sub["mesh"], engine)
    before = {k: np.array(x, copy=True) for k, x in res.items() if isinstance(x, np.ndarray)}
    got = mm.create_wall_mesh(None, cla, clr, cl_l, res, aortic_scaling=1.25, coronary_scaling=0.5, engine=engine)
    wv, wf, wrep = CM.create_wall_mesh(dict(res), ca, cr, cll, 1.25, 0.5)
    gv, gf = got["mesh"]
    assert same_bits(gv, wv) and np.array_equal(gf, wf)
    assert got is not res and "wall_report" not in res and all(np.array_equal(res[k], x) for k, x in before.items())
    rep = got["wall_report"]
    assert rep["aortic_scaling"] == 1.25 and rep["coronary_scaling"] == 0.5
    for k in FILL_KEYS:
        assert rep["fill_report"][k] == wrep[k], k
    assert rep["fill_report"]["n_open_edges"] == 0                         # the aortic part is closed
    n_aorta_faces = rep["fill_report"]["n_faces"]
    assert CM.SM.face_adjacency(gf[:n_aorta_faces])[1] == 0
    # the scaling derived from a geometry: the same composition with find_aortic_wall_scaling's value
    _, geom, _ = takeoff_case(engine)
    scaling = mm.find_aortic_wall_scaling(geom, cla, res)
    got = mm.create_wall_mesh(geom, cla, clr, cl_l, res, engine=engine)
    wv, wf, _ = CM.create_wall_mesh(dict(res), ca, cr, cll, scaling, 1.0)
    assert got["wall_report"]["aortic_scaling"] == scaling
    assert same_bits(got["mesh"][0], wv) and np.array_equal(got["mesh"][1], wf)
    with pytest.raises(ValueError, match="lca_points"):
        mm.create_wall_mesh(None, cla, clr, cl_l, dict(res, lca_points=np.zeros((0, 3))), aortic_scaling=1.0, engine=engine)
