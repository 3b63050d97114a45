"""CCTA stitching on the device (csrc/mm_weld_kernels.hip, csrc/mm_stitch.cpp) against the checker
(tests/mm_checkers/stitch_mesh.py): identical indices, bit-identical coordinates and volume.  Winding on closed meshes
with every subset (octahedron) or seeded subsets (capped tube) of faces reversed, two bodies, a boundary, a non-manifold
fin, a Moebius strip beside an orientable body, overlapping parts, random meshes with degenerate, repeated and
index-permuted repeated faces on a coarse coordinate grid (thousands of keys in a half-full table: probing happens), the
weld rules, a thin tube of 10^6 faces whose launch count must stay within the bound of DESIGN 4.12, an inside-out body,
and the pipeline label -> remove(target_boundaries=2) -> stitch on the synthetic take-off mesh."""
import itertools
import math

import numpy as np
import pytest

from mm_checkers import stitch_mesh as K
from test_trim_host import octahedron, capped_tube
from test_stitch_host import RUST_CASES, edge_counts, icosahedron, same_bits

import multimoda_rs_amd as mm

pytestmark = pytest.mark.gpu

REPORT_KEYS = ("n_vertices", "n_faces", "n_welded_vertices", "n_unreferenced_vertices", "n_degenerate_faces",
               "n_duplicate_faces", "n_flipped_faces", "n_winding_conflicts", "n_open_edges", "n_nonmanifold_edges",
               "inverted", "watertight")


def round_bound(nf):
    return 2 + math.ceil(math.log2(max(nf, 2)))


def same_assembly(parts, engine, digits=3, wind=True, inv=True):
    gv, gf, gr = mm.assemble_mesh(parts, digits, wind, inv, engine=engine)
    wv, wf, wr = K.assemble([mm.ccta._mesh_parts(p) for p in parts], digits, wind, inv)
    assert same_bits(gv, wv)
    assert np.array_equal(gf, wf)
    for k in REPORT_KEYS:
        assert gr[k] == wr[k], (k, gr[k], wr[k])
    assert np.float64(gr["volume"]).view(np.uint64) == np.float64(wr["volume"]).view(np.uint64), (gr["volume"], wr["volume"])
    assert (gr["winding_rounds"] == 0) if (not wind or wr["n_faces"] == 0) else (1 < gr["winding_rounds"] <= round_bound(wr["n_faces"]))
    return gv, gf, gr


def reversed_subset(f, mask):
    g = np.array(f, dtype=np.int64)
    g[mask] = g[mask][:, ::-1]
    return g


def thin_tube(n_rings, n_around=4, radius=1.0):
    c = np.stack([np.zeros(n_rings), np.zeros(n_rings), 0.25 * np.arange(n_rings, dtype=float)], 1)
    return mm.synth._tube(c, np.tile([1.0, 0, 0], (n_rings, 1)), np.tile([0, 1.0, 0], (n_rings, 1)), radius, n_around)


def moebius(n=24):
    """A closed strip of n quads with a half twist: every inner edge has two owners, and no orientation exists."""
    t = np.linspace(0, 2 * np.pi, n, endpoint=False)
    a = np.stack([(3 + np.cos(t / 2)) * np.cos(t), (3 + np.cos(t / 2)) * np.sin(t), np.sin(t / 2)], 1)
    b = np.stack([(3 - np.cos(t / 2)) * np.cos(t), (3 - np.cos(t / 2)) * np.sin(t), -np.sin(t / 2)], 1)
    ia = lambda i: i if i < n else n + (i - n)                                      # noqa: E731  a_n = b_0
    ib = lambda i: n + i if i < n else i - n                                        # noqa: E731  b_n = a_0
    f = []
    for i in range(n):
        f.append([ia(i), ia(i + 1), ib(i)])
        f.append([ia(i + 1), ib(i + 1), ib(i)])
    return np.concatenate([a, b]), np.array(f, dtype=np.int64)


def messy_mesh(seed, nv=6000, nf=20000):
    """Faces on a random index pattern over a coarse coordinate grid (many shared keys), with degenerate faces, repeated
    faces and repeated faces with their indices permuted."""
    r = np.random.default_rng(seed)
    v = np.round(r.normal(size=(nv, 3)) * 0.5, 1)
    v[r.integers(0, nv, 50)] = -0.0
    base = r.integers(0, nv - 3, nf)
    f = np.stack([base, base + r.integers(1, 3, nf), base + 3], 1)
    f[:200, 1] = f[:200, 0]
    f[200:500] = f[1000:1300]
    f[500:800] = f[1300:1600][:, [1, 2, 0]]
    f[800:1000] = f[1600:1800][:, [2, 1, 0]]
    return v, f[r.permutation(nf)]


# ---- fix_mesh_winding ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("faces, want", RUST_CASES)
def test_fix_mesh_winding_rust_cases(engine, faces, want):
    got = mm.fix_mesh_winding(np.array(faces, dtype=np.int64).reshape(-1, 3), engine=engine)
    assert got.tolist() == want and got.dtype == np.int64


def test_octahedron_every_subset_reversed(engine):
    _, f = octahedron()
    for bits in itertools.product([False, True], repeat=len(f)):
        g = reversed_subset(f, np.array(bits))
        got = mm.fix_mesh_winding(g, engine=engine)
        want = K.fix_winding(g)[0]
        assert np.array_equal(got, want), bits
        assert np.array_equal(got, f if not bits[0] else f[:, ::-1])


def test_capped_tube_seeded_subsets_and_the_whole_assembly(engine):
    v, f = capped_tube(12, 9)
    r = np.random.default_rng(11)
    for _ in range(40):
        g = reversed_subset(f, r.random(len(f)) < r.random())
        got, info = mm.ccta._fix_winding(g, engine)
        want, flipped, conflicts = K.fix_winding(g)
        assert np.array_equal(got, want) and info["n_flipped_faces"] == flipped.sum() and info["n_winding_conflicts"] == 0
        assert 1 < info["winding_rounds"] <= round_bound(len(f))
        _, of, rep = same_assembly([(v, g)], engine)
        assert rep["watertight"] and K.pair_tree_sum(K.volume_terms(v, of)) > 0


def test_two_bodies_boundary_and_fin(engine):
    v, f = octahedron()
    tv, tf = capped_tube(8, 5)
    r = np.random.default_rng(3)
    for _ in range(10):
        parts = [(v + [10.0, 0, 0], reversed_subset(f, r.random(len(f)) < 0.5)),
                 (tv, reversed_subset(tf, r.random(len(tf)) < 0.5))]
        _, _, rep = same_assembly(parts, engine)
        assert rep["watertight"] and rep["n_winding_conflicts"] == 0
    open_tube = tf[:-8]                                                # one cap missing: a boundary
    _, _, rep = same_assembly([(tv, reversed_subset(open_tube, r.random(len(open_tube)) < 0.5))], engine)
    assert rep["n_open_edges"] == 8 and not rep["watertight"]
    # a fin on edge {0, 2}, wound against its neighbours: the edge has three owners and carries no parity
    fv = np.concatenate([v, [[2.0, 2.0, 0.0]]])
    g = np.concatenate([f, [[2, 0, 6]]])
    got = mm.fix_mesh_winding(g, engine=engine)
    assert np.array_equal(got, g) and np.array_equal(got, K.fix_winding(g)[0])
    _, _, rep = same_assembly([(fv, g)], engine, inv=False)
    assert rep["n_nonmanifold_edges"] == 1 and rep["n_open_edges"] == 2 and rep["n_flipped_faces"] == 0


def test_moebius_strip_beside_an_orientable_body(engine):
    mv, mf = moebius()
    v, f = octahedron()
    g = reversed_subset(f, np.array([0, 1, 1, 0, 1, 0, 0, 1], dtype=bool))
    assert K.fix_winding(mf)[2] > 0
    ov, of, rep = mm.assemble_mesh([(v + [20.0, 0, 0], g), (mv, mf)], fix_inversion=False, engine=engine)
    wv, wf, wrep = K.assemble([(v + [20.0, 0, 0], g), (mv, mf)], 3, True, False)
    assert rep["n_winding_conflicts"] > 0 and wrep["n_winding_conflicts"] > 0
    assert same_bits(ov, wv) and np.array_equal(of[:8], wf[:8]) and np.array_equal(of[:8], f)
    assert np.array_equal(np.sort(of, axis=1), np.sort(wf, axis=1))    # the strip: the same faces, flips unspecified
    assert rep["winding_rounds"] <= round_bound(len(of))


def test_overlapping_parts_share_a_ring(engine):
    v, f = capped_tube(16, 9)
    lower, upper = f[(v[f][:, :, 2] <= 4).all(axis=1)], f[(v[f][:, :, 2] >= 4).all(axis=1)]
    r = np.random.default_rng(9)
    parts = [(v, reversed_subset(lower, r.random(len(lower)) < 0.5)), (v.copy() + [0, 0, 2e-4], upper)]
    _, of, rep = same_assembly(parts, engine)
    assert rep["watertight"] and rep["n_welded_vertices"] == 16 and len(of) == len(f)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_messy_meshes(engine, seed):
    v, f = messy_mesh(seed)
    _, _, rep = same_assembly([(v, f)], engine, wind=False)
    assert rep["n_degenerate_faces"] >= 200 and rep["n_duplicate_faces"] >= 800 and rep["n_welded_vertices"] > 100
    same_assembly([(v, f[:7000]), (v[::-1].copy(), f[7000:])], engine, digits=0, wind=False)
    # with the winding stage the faces and every count but the flips are still pinned
    gv, gf, gr = mm.assemble_mesh([(v, f)], engine=engine)
    wv, wf, wr = K.assemble([(v, f)])
    assert same_bits(gv, wv) and np.array_equal(np.sort(gf, axis=1), np.sort(wf, axis=1))
    for k in ("n_welded_vertices", "n_degenerate_faces", "n_duplicate_faces", "n_open_edges", "n_nonmanifold_edges"):
        assert gr[k] == wr[k]
    if wr["n_winding_conflicts"] == 0:
        assert gr["n_winding_conflicts"] == 0 and np.array_equal(gf, wf)


WELD_CASES = [
    ([[0.5, 0, 0], [0.0, 0, 0], [1.5, 0, 0], [2.0, 0, 0], [2.5, 0, 0], [9, 9, 9], [8, 8, 8]],
     [[0, 5, 6], [1, 5, 6], [2, 5, 6], [3, 5, 6], [4, 5, 6]], 0),
    ([[x, 0, 0] for x in (0.0005, 0.0015, 0.0025, 2.0005, 2.0015, 0.0, 0.001, 0.002, 2.0, 2.001, 2.002)] +
     [[5, 5, 5], [6, 6, 6]], [[i, 11, 12] for i in range(11)], 3),
    ([[-0.0, 0, 0], [0.0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 2, 3], [1, 3, 2]], 3),
    ([[float("nan"), 0, 0], [float("nan"), 0, 0], [1e300, 0, 0], [1e300, 0, 0], [float("inf"), 0, 0],
      [float("inf"), 0, 0], [4.6e15, 0, 0], [4.6e15, 0, 0], [1, 0, 0], [0, 1, 0]],
     [[i, 8, 9] for i in range(8)], 3),
    ([[1, 1, 1], [0, 0, 0], [1, 1, 1], [2, 0, 0], [0, 2, 0]], [[2, 3, 4], [1, 3, 4]], 3),
    ([[0.0101, 0, 0], [0.0103, 0, 0], [0.0104, 0, 0], [5, 5, 5], [6, 6, 6]], [[0, 3, 4], [1, 3, 4], [2, 3, 4]], 3),
    ([[0.0101, 0, 0], [0.0104, 0, 0], [0.0107, 0, 0], [5, 5, 5], [6, 6, 6]], [[0, 3, 4], [1, 3, 4], [2, 3, 4]], 3),
    (octahedron()[0].tolist(), [[0, 2, 4], [4, 0, 2], [2, 0, 4], [0, 0, 4], [2, 1, 4]], 3),
]


@pytest.mark.parametrize("case", range(len(WELD_CASES)))
def test_weld_rules(engine, case):
    v, f, digits = WELD_CASES[case]
    for wind, inv in ((False, False), (True, True)):
        same_assembly([(np.array(v, dtype=float), np.array(f))], engine, digits, wind, inv)


def test_empty_and_faceless_inputs(engine):
    v, f, rep = mm.assemble_mesh([], engine=engine)
    assert v.shape == (0, 3) and f.shape == (0, 3) and rep["watertight"]
    v, f, rep = mm.assemble_mesh([(octahedron()[0], np.zeros((0, 3), dtype=np.int64))], engine=engine)
    assert v.shape == (0, 3) and rep["n_unreferenced_vertices"] == 6
    same_assembly([(octahedron()[0], [[0, 0, 1]])], engine)           # every face degenerate
    assert mm.fix_mesh_winding([], engine=engine).shape == (0, 3)


def test_inside_out_body(engine):
    v, f = icosahedron()
    ov, of, rep = same_assembly([(v, f[:, ::-1])], engine)
    assert rep["inverted"] == 1 and rep["volume"] < 0 and np.array_equal(of, f)
    _, of, rep = same_assembly([(v, f)], engine)
    assert rep["inverted"] == 0 and rep["volume"] > 0 and np.array_equal(of, f)


def test_rejections(engine):
    v, f = octahedron()
    with pytest.raises(ValueError):
        mm.assemble_mesh([(v, f + 1)], engine=engine)
    with pytest.raises(RuntimeError):
        mm.assemble_mesh([(v, f)], merge_digits=16, engine=engine)
    with pytest.raises(ValueError):
        mm.fix_mesh_winding([[0, 1, -2]], engine=engine)
    L, N = mm._native.lib(), mm._native
    bad = np.array([[0, 1, 6]], dtype=np.int64)
    off_v, off_f = np.array([0, 6], dtype=np.int64), np.array([0, 1], dtype=np.int64)
    rep = N.MMAssembleReport()
    import ctypes as C
    out_v, out_f = np.zeros((6, 3)), np.zeros((1, 3), dtype=np.int64)
    assert L.mm_mesh_assemble(engine.handle, 1, N._ptr(v), N._ptr(off_v), N._ptr(bad), N._ptr(off_f), 3, 1, 1,
                              N._ptr(out_v), N._ptr(out_f), C.byref(rep)) == -2
    assert "face index out of range" in N.last_error()


def test_a_million_faces_thin_tube(engine):
    v, f = thin_tube(125001, 4)
    assert f.shape[0] >= 10 ** 6
    r = np.random.default_rng(2)
    g = reversed_subset(f, r.random(len(f)) < 0.5)
    got, info = mm.ccta._fix_winding(g, engine)
    want, flipped, conflicts = K.fix_winding(g)
    assert np.array_equal(got, want) and conflicts == 0 and info["n_winding_conflicts"] == 0
    assert info["n_flipped_faces"] == int(flipped.sum())
    # the face-adjacency diameter is of the order of 125 000; the launches stay logarithmic
    assert 1 < info["winding_rounds"] <= round_bound(len(f)) == 22, info
    _, _, rep = same_assembly([(v, g)], engine)
    assert rep["n_open_edges"] == 8 and rep["winding_rounds"] <= 22


# ---- pipeline -----------------------------------------------------------------------------------------------------------

def cl_of(xyz):
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    a = np.zeros(xyz.shape[0], dtype=mm.centerline.CL_DTYPE)
    a["x"], a["y"], a["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return mm.Centerline(a)


def takeoff_case(engine):
    v, f, ca, cr, cll, _ = mm.synth.synthetic_takeoff_mesh()
    cla, clr, cl_l = cl_of(ca), cl_of(cr), cl_of(cll)
    res = mm.label_geometry((v, f), cla, clr, cl_l, acute_takeoff_rca=True, engine=engine)
    n_around = 16
    na = v.shape[0] - 2 * len(cr) * n_around
    lo, hi = 24, 48
    tube_ring = lambda k: v[na + k * n_around: na + (k + 1) * n_around]             # noqa: E731
    res["section_points"] = np.concatenate([tube_ring(k) for k in range(lo, hi + 1)])
    frames = []
    for k in range(lo, hi + 1):                                       # the IV lumen: the cut rings, narrower, 32 points
        ring = tube_ring(k)
        c = ring.mean(axis=0)
        fine = np.empty((2 * n_around, 3))
        fine[0::2] = ring
        fine[1::2] = 0.5 * (ring + np.roll(ring, -1, axis=0))
        frames.append(c + 0.8 * (fine - c))
    return res, mm.FlatGeometry.from_frames(frames), frames


@pytest.mark.parametrize("modes", [("nearest_iv", "nearest_iv"), ("highest_z", "nearest_iv"), ("highest_z", "highest_z")])
@pytest.mark.parametrize("n_iv", [100, 24])
def test_pipeline_label_remove_stitch(engine, modes, n_iv):
    res, geom, frames = takeoff_case(engine)
    cut = mm.remove_labeled_points_from_mesh(dict(res), "section_points", target_boundaries=2, engine=engine)
    assert "boundary_points_2" in cut
    got = mm.stitch_ccta_to_intravascular(geom, cut["mesh"], cut, n_points_iv_cont=n_iv, prox_start_mode=modes[0],
                                          dist_start_mode=modes[1], engine=engine)
    rings = [cut["boundary_points_1"], cut["boundary_points_2"]]
    parts, prox_b, dist_b = K.stitch_parts(frames, geom.centroids, geom.centroids[0], rings, cut["mesh"], n_iv, *modes)
    wv, wf, wr = K.assemble(parts)
    gv, gf = got["mesh"]
    assert same_bits(gv, wv) and np.array_equal(gf, wf)
    assert same_bits(got["prox_boundary_points"], prox_b) and same_bits(got["dist_boundary_points"], dist_b)
    rep = got["stitch_report"]
    for k in REPORT_KEYS:
        assert rep[k] == wr[k], k
    assert np.float64(rep["volume"]).view(np.uint64) == np.float64(wr["volume"]).view(np.uint64)
    assert rep["n_winding_conflicts"] == 0 and rep["n_nonmanifold_edges"] == 0
    assert set(got) >= {"prox_boundary_points", "dist_boundary_points", "anomalous_points", "rca_points", "mesh"}
    assert len(got["anomalous_points"]) == len(frames) * min(n_iv, 32)
    # every strip edge has two owners, and no vertex of the two stitched rims is left on an open edge
    counts = edge_counts(gf)
    open_vertices = {i for e, c in counts.items() if c == 1 for i in e}
    for b, iv_ring in ((prox_b, parts[1][0][len(prox_b):]), (dist_b, parts[2][0][len(dist_b):])):
        strip_v = np.concatenate([b, iv_ring])
        idx = mm.ccta._match(gv, strip_v)
        assert (idx >= 0).all() and not (set(idx.tolist()) & open_vertices)
    for pv, pf in (parts[1], parts[2]):
        idx = mm.ccta._match(gv, pv)
        for e in edge_counts(idx[pf]).keys():
            assert counts[e] == 2, e


def test_stitch_wrapper_and_ring_fallback(engine):
    res, geom, frames = takeoff_case(engine)
    got = mm.stitch(dict(res), geom, region_remove="section_points", engine=engine)
    cut = mm.remove_labeled_points_from_mesh(dict(res), "section_points", target_boundaries=2, engine=engine)
    want = mm.stitch_ccta_to_intravascular(geom, cut["mesh"], cut, prox_start_mode="highest_z", engine=engine)
    assert same_bits(got["mesh"][0], want["mesh"][0]) and np.array_equal(got["mesh"][1], want["mesh"][1])
    # without the per-ring keys the rings come from the mesh's open edges that hold a boundary point
    flat = {k: v for k, v in cut.items() if not k.startswith("boundary_points_")}
    again = mm.stitch_ccta_to_intravascular(geom, cut["mesh"], flat, prox_start_mode="highest_z", engine=engine)
    assert again["stitch_report"]["n_faces"] == want["stitch_report"]["n_faces"]
    assert again["stitch_report"]["n_open_edges"] == want["stitch_report"]["n_open_edges"]
    with pytest.raises(ValueError, match="target_boundaries=2"):
        mm.stitch_ccta_to_intravascular(geom, cut["mesh"], {"boundary_points_1": cut["boundary_points_1"]}, engine=engine)
