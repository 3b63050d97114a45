"""Mesh refinement on the device (csrc/mm_refine_kernels.hip, csrc/mm_refine.cpp) against the checker
(tests/mm_checkers/refine_mesh.py): identical faces and parents, bit-identical vertices, equal integer report fields
(the splits per pass, the faces by template, the launch and byte counts), bit-equal longest squared lengths and volumes.
Shapes: the small solids, the stretched tube (all four templates over several passes), meshes one vertex past a
workgroup (257) and past a scan tile (4097), an open tube, a target nothing reaches, 0 and 1 passes, the vertex cap,
capacities one too small, shuffled faces, a messy face list, random meshes, the argument checks, and the line label ->
remove -> stitch(fill_holes=True, refine=True, smooth=True)."""
import ctypes as C
import os

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings, strategies as st

from mm_checkers import refine_mesh as R
from mm_checkers import stitch_mesh as SM
from test_trim_host import octahedron, capped_tube
from test_smooth_host import tetrahedron
from test_refine_host import same_bits, jitter, stretched_tube, open_tube, messy, wound_tube
from test_gpu_stitch import takeoff_case

import multimoda_rs_amd as mm
from multimoda_rs_amd import ccta

pytestmark = pytest.mark.gpu

N = mm._native
MM_ERR_INVALID, MM_ERR_TOO_LARGE = -2, -3
INT_KEYS = ("n_vertices", "n_faces", "n_edges_before", "n_edges_after", "passes_run", "converged", "stopped_by_cap",
            "n_open_edges_before", "n_open_edges_after", "n_nonmanifold_edges_before", "n_nonmanifold_edges_after",
            "n_launches", "bytes_uploaded", "bytes_downloaded", "splits_per_pass", "faces_by_template")
F64_KEYS = ("longest_sq_before", "longest_sq_after", "volume_before", "volume_after")


def bits_equal(a, b):
    return np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


def same_refine(v, f, L, engine, **kw):
    mesh, parents, rep = mm.refine_mesh((v, f), L, engine=engine, **kw)
    ckw = {"max_passes": kw.get("passes", 10), "max_vertices": kw.get("max_vertices"), "ratio": kw.get("ratio", 4.0 / 3.0)}
    wv, wf, wp, wrep = R.refine(v, f, L, **ckw)
    assert mesh[1].dtype == np.int64 and np.array_equal(mesh[1], wf) and np.array_equal(parents, wp)
    assert same_bits(mesh[0], wv)
    for k in INT_KEYS:
        assert rep[k] == wrep[k], (k, rep[k], wrep[k])
    for k in F64_KEYS:
        assert bits_equal(rep[k], wrep[k]), (k, rep[k], wrep[k])
    assert rep["target_edge_length_mm"] == L and rep["threshold_mm"] == kw.get("ratio", 4.0 / 3.0) * L
    edges, lengths = mm.mesh_edge_lengths((v, f), engine=engine)
    wedges, wlen_sq = R.edge_lengths(v, f)
    assert np.array_equal(edges, wedges) and same_bits(lengths, np.sqrt(wlen_sq))
    return mesh, parents, rep


@pytest.mark.parametrize("solid", [tetrahedron, octahedron])
def test_small_solids(engine, solid):
    v, f = solid()
    _, _, rep = same_refine(v, f, 0.3, engine)
    assert rep["converged"] == 1 and rep["watertight"]
    if solid is octahedron:
        assert rep["splits_per_pass"][:3] == [12, 48, 0] and rep["n_vertices"] == 66 and rep["n_faces"] == 128
        assert rep["n_launches"] == 6 + 6 + 4 + 2 + 2
    same_refine(jitter(v, 1), f, 0.5, engine)


def test_stretched_tube_uses_all_four_templates(engine):
    v, f = stretched_tube()
    _, _, rep = same_refine(v, f, 0.3, engine)
    assert rep["splits_per_pass"][:5] == [108, 288, 576, 1728, 0]
    _, _, rep = same_refine(jitter(v, 3), f, 0.25, engine)
    assert all(n > 0 for n in rep["faces_by_template"]) and rep["passes_run"] >= 4


def test_one_vertex_past_a_workgroup(engine):
    v, f = capped_tube(15, 17)
    assert len(v) == 257
    same_refine(v, f, 0.4, engine)
    same_refine(jitter(v, 17), f, 0.4, engine)


def test_one_vertex_past_a_scan_tile_split_in_part(engine):
    v, f = capped_tube(63, 65)
    assert len(v) == 4097 and len(f) > 4096
    # the edges are 4095 around the rings (0.0997), 4158 along the axis and in the caps (1.0) and 4032 diagonals
    # (sqrt(1 + 0.0997^2) = 1.005).  A threshold of 4/3 * 0.752 = 1.0027 lies between the last two: only the diagonals
    # split, one edge of every wall face; 4/3 * 0.5 takes the axial edges too, two edges of every face
    _, _, rep = same_refine(v, f, 0.752, engine)
    assert rep["splits_per_pass"][:2] == [4032, 0] and rep["n_edges_before"] == 12285
    assert rep["faces_by_template"][1] == 2 * 4032 and rep["faces_by_template"][2:] == [0, 0]
    _, _, rep = same_refine(v, f, 0.5, engine)
    assert rep["splits_per_pass"][:2] == [4158 + 4032, 0] and rep["faces_by_template"][1:] == [0, 2 * 4032 + 126, 0]


def test_open_tube(engine):
    v, f = open_tube()
    _, _, rep = same_refine(v, f, 0.3, engine)
    assert rep["n_open_edges_before"] == 30 < rep["n_open_edges_after"] and not rep["watertight"]


def test_a_target_nothing_reaches(engine):
    v, f = jitter(capped_tube(15, 17)[0], 2), capped_tube(15, 17)[1]
    mesh, parents, rep = same_refine(v, f, 10.0, engine)
    assert same_bits(mesh[0], v) and np.array_equal(mesh[1], f) and len(parents) == 0
    assert rep["splits_per_pass"][0] == 0 and rep["converged"] == 1 and rep["passes_run"] == 1


@pytest.mark.parametrize("passes", [0, 1, 2])
def test_pass_counts(engine, passes):
    v, f = octahedron()
    mesh, _, rep = same_refine(v, f, 0.3, engine, passes=passes)
    assert rep["passes_run"] == passes and rep["converged"] == 0 and len(mesh[0]) == (6, 18, 66)[passes]
    if passes == 0:
        assert same_bits(mesh[0], v) and rep["n_launches"] == 2 + 2 * 2


def test_vertex_cap_stops_in_front_of_the_second_pass(engine):
    v, f = octahedron()
    mesh, _, rep = same_refine(v, f, 0.3, engine, max_vertices=65)
    assert rep["stopped_by_cap"] == 1 and rep["passes_run"] == 1 and len(mesh[0]) == 18 and len(mesh[1]) == 32
    _, _, rep = same_refine(v, f, 0.3, engine, max_vertices=66)
    assert rep["stopped_by_cap"] == 0 and rep["converged"] == 1


def _raw(engine, v, f, L, vert_cap, face_cap, handle=True, passes=10):
    v = np.ascontiguousarray(v, dtype=np.float64)
    f = np.ascontiguousarray(f, dtype=np.int64)
    out = {"v": np.full((vert_cap, 3), 7.5), "f": np.full((face_cap, 3), -77, dtype=np.int64),
           "p": np.full((max(vert_cap - len(v), 1), 2), -77, dtype=np.int64)}
    rep = N.MMRefineReport()
    C.memset(C.byref(rep), 0x5A, C.sizeof(rep))
    rc = N.lib().mm_mesh_refine(engine.handle if handle else None, N._ptr(v), len(v), N._ptr(f), len(f), L, 4.0 / 3.0,
                                passes, 2 ** 31 - 1, vert_cap, face_cap, N._ptr(out["v"]), N._ptr(out["f"]),
                                N._ptr(out["p"]), C.byref(rep))
    return rc, out, rep


def untouched(out):
    return (out["v"] == 7.5).all() and (out["f"] == -77).all() and (out["p"] == -77).all()


def test_capacities_one_too_small(engine):
    v, f = octahedron()
    for vert_cap, face_cap in ((65, 128), (66, 127)):
        rc, out, rep = _raw(engine, v, f, 0.3, vert_cap, face_cap)
        assert rc == MM_ERR_TOO_LARGE and untouched(out) and rep.n_vertices == 66 and rep.n_faces == 128
        assert list(rep.splits_per_pass)[:3] == [12, 48, 0] and rep.bytes_downloaded == 0
    rc, out, rep = _raw(engine, v, f, 0.3, 66, 128)
    wv, wf, wp, _ = R.refine(v, f, 0.3)
    assert rc == 0 and same_bits(out["v"], wv) and np.array_equal(out["f"], wf) and np.array_equal(out["p"], wp)
    # the edge list: one too small, then exact
    edges, len_sq, info = np.full((11, 2), -77, dtype=np.int64), np.full(11, 7.5), np.zeros(4, dtype=np.int64)
    fi = np.ascontiguousarray(f, dtype=np.int64)
    call = lambda cap: N.lib().mm_mesh_edge_lengths(engine.handle, N._ptr(v), 6, N._ptr(fi), 8, cap, N._ptr(edges),       # noqa: E731
                                                    N._ptr(len_sq), N._ptr(info))
    assert call(11) == MM_ERR_TOO_LARGE and info.tolist() == [12, 0, 0, 4] and (edges == -77).all() and (len_sq == 7.5).all()
    edges, len_sq = np.zeros((12, 2), dtype=np.int64), np.zeros(12)
    assert call(12) == 0 and info.tolist() == [12, 0, 0, 5] and (len_sq == 2.0).all()


def test_shuffled_faces_change_the_result_and_still_equal_the_checker(engine):
    v, f = stretched_tube()
    v = jitter(v, 3)
    base, _, _ = same_refine(v, f, 0.25, engine)
    r = np.random.default_rng(5)
    g = f[r.permutation(len(f))]
    g = np.stack([np.roll(t, int(k)) for t, k in zip(g, r.integers(0, 3, len(g)))])
    other, _, rep = same_refine(v, g, 0.25, engine)
    assert other[0].shape == base[0].shape and not same_bits(other[0], base[0])       # another numbering
    key = lambda a: np.sort(a.view([("", a.dtype)] * 3).ravel())                      # noqa: E731
    assert np.array_equal(key(np.ascontiguousarray(other[0])), key(np.ascontiguousarray(base[0])))   # of the same points


def test_messy_face_list(engine):
    v, f = messy()
    for L in (0.6, 1.0, 5.0):
        _, _, rep = same_refine(v, f, L, engine)
    assert rep["n_nonmanifold_edges_before"] == 1
    same_refine(v, f, 0.6, engine, passes=2)
    empty = np.zeros((0, 3), dtype=np.int64)
    mesh, parents, rep = mm.refine_mesh((v, empty), 0.5, engine=engine)
    assert same_bits(mesh[0], v) and mesh[1].shape == (0, 3) and len(parents) == 0 and rep["n_launches"] == 0
    assert R.refine(v, empty, 0.5)[3]["n_launches"] == 0
    with pytest.raises(ValueError, match="no edge"):
        mm.refine_mesh((v, empty), engine=engine)


@settings(max_examples=40 * int(os.environ.get("MM_HYP_SCALE", "1")), deadline=None, derandomize=True, database=None,
          suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(seed=st.integers(0, 2**31 - 1), nv=st.integers(1, 40), nf=st.integers(0, 50), passes=st.integers(0, 3),
       L=st.sampled_from([0.8, 1.5, 3.0]), cap=st.sampled_from([None, 60, 200]))
def test_random_small_meshes(engine, seed, nv, nf, passes, L, cap):
    r = np.random.default_rng(seed)
    v = r.uniform(-3, 3, (nv, 3))
    f = r.integers(0, nv, (nf, 3))
    same_refine(v, f, L, engine, passes=passes, max_vertices=cap)


def test_default_target_is_the_25th_percentile(engine):
    v, f = stretched_tube()
    v = jitter(v, 5)
    _, len_sq = R.edge_lengths(v, f)
    want = float(np.percentile(np.sqrt(len_sq), 25.0))
    assert mm.edge_length_target((v, f), engine=engine) == want
    mesh, parents, rep = mm.refine_mesh((v, f), engine=engine, passes=2)
    wv, wf, wp, _ = R.refine(v, f, want, max_passes=2)
    assert rep["target_edge_length_mm"] == want and same_bits(mesh[0], wv) and np.array_equal(mesh[1], wf)

    class Mesh:
        def __init__(self, vertices, faces):
            self.vertices, self.faces = vertices, faces

    src = Mesh(v.copy(), f.copy())
    m, _, _ = mm.refine_mesh(src, want, passes=2, engine=engine)
    assert isinstance(m, Mesh) and m is not src and same_bits(m.vertices, wv) and np.array_equal(m.faces, wf)
    assert same_bits(src.vertices, v) and np.array_equal(src.faces, f)                 # the input is not modified


# ---- the argument checks of tests/test_gpu_mesh_args.py, for the two functions that name their triangles `tris` -------

def test_face_index_out_of_range_and_null_engine(engine):
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0]])
    bad = np.array([[0, 1, 2], [0, 2, 4]], dtype=np.int64)
    for handle, err in ((True, "mm_mesh_refine: face index out of range"), (False, "engine == NULL")):
        rc, out, rep = _raw(engine, v, bad, 0.3, 16, 16, handle=handle)
        assert rc == MM_ERR_INVALID and N.last_error() == err and untouched(out)
        assert (np.frombuffer(rep, dtype=np.uint8) == 0x5A).all()
    edges, len_sq, info = np.full((8, 2), -77, dtype=np.int64), np.full(8, 7.5), np.full(4, -77, dtype=np.int64)
    for handle, err in ((engine.handle, "mm_mesh_edge_lengths: face index out of range"), (None, "engine == NULL")):
        rc = N.lib().mm_mesh_edge_lengths(handle, N._ptr(v), 4, N._ptr(bad), 2, 8, N._ptr(edges), N._ptr(len_sq), N._ptr(info))
        assert rc == MM_ERR_INVALID and N.last_error() == err
        assert (edges == -77).all() and (len_sq == 7.5).all() and (info == -77).all()
    good = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int64)
    for L, ratio, passes in ((0.0, 1.0, 1), (-1.0, 1.0, 1), (float("nan"), 1.0, 1), (1.0, float("inf"), 1), (1e-300, 1e-300, 1),
                             (1e300, 1e300, 1), (1.0, 1.0, -1)):
        out_v, out_f, out_p = np.zeros((16, 3)), np.zeros((16, 3), dtype=np.int64), np.zeros((12, 2), dtype=np.int64)
        rep = N.MMRefineReport()
        rc = N.lib().mm_mesh_refine(engine.handle, N._ptr(v), 4, N._ptr(good), 2, L, ratio, passes, 100, 16, 16, N._ptr(out_v),
                                    N._ptr(out_f), N._ptr(out_p), C.byref(rep))
        assert rc == MM_ERR_INVALID, (L, ratio, passes)


# ---- the line label -> remove -> stitch ---------------------------------------------------------------------------------

def test_stitch_with_and_without_refinement(engine):
    res, geom, frames = takeoff_case(engine)
    plain = mm.stitch(dict(res), geom, region_remove="section_points", engine=engine, fill_holes=True)
    again = mm.stitch(dict(res), geom, region_remove="section_points", engine=engine, fill_holes=True, refine=False)
    assert "refine_report" not in plain and sorted(plain) == sorted(again)
    assert same_bits(plain["mesh"][0], again["mesh"][0]) and np.array_equal(plain["mesh"][1], again["mesh"][1])
    assert plain["fill_report"]["watertight"]

    fine = mm.stitch(dict(res), geom, region_remove="section_points", engine=engine, fill_holes=True, refine=True,
                     smooth=True)
    want, parents, wrep = mm.refine_mesh(plain["mesh"], engine=engine)
    assert fine["refine_report"] == wrep and wrep["watertight"] and wrep["converged"] == 1 and len(parents) > 0
    assert wrep["n_open_edges_before"] == 0 and wrep["n_nonmanifold_edges_before"] == 0
    cv, cf, cp, crep = R.refine(*plain["mesh"], wrep["target_edge_length_mm"])
    assert same_bits(want[0], cv) and np.array_equal(want[1], cf) and np.array_equal(parents, cp)
    _, n_open, n_nonmanifold = SM.face_adjacency(fine["mesh"][1])
    assert n_open == 0 and n_nonmanifold == 0 and np.array_equal(fine["mesh"][1], want[1])
    smoothed, srep = mm.smooth_mesh(want, engine=engine)
    assert same_bits(fine["mesh"][0], smoothed[0]) and fine["smooth_report"] == srep

    # without the smoothing: no vertex of the IV lumen (nor any other) moved, and the lists sit on the mesh
    only = mm.stitch(dict(res), geom, region_remove="section_points", engine=engine, fill_holes=True, refine=True)
    nv0 = len(plain["mesh"][0])
    assert same_bits(only["mesh"][0], want[0]) and same_bits(only["mesh"][0][:nv0], plain["mesh"][0])
    iv = plain["anomalous_points"]                                        # the IV lumen as stitched
    at = ccta._match(plain["mesh"][0], iv)
    assert (at >= 0).sum() > 0 and same_bits(only["mesh"][0][at[at >= 0]], iv[at >= 0])
    grown = 0
    for key in ccta.SYNC_KEYS:
        if key in plain and len(plain[key]):
            n = len(plain[key])
            assert same_bits(only[key][:n], plain[key])                   # the list as it was, then the new vertices
            member = np.zeros(len(only["mesh"][0]), dtype=bool)
            member[:nv0] = ccta._match(plain[key], plain["mesh"][0]) >= 0
            for k in range(len(parents)):                                 # ascending: both parents in the list
                member[nv0 + k] = member[parents[k, 0]] and member[parents[k, 1]]
            assert same_bits(only[key][n:], only["mesh"][0][nv0:][member[nv0:]])
            assert (ccta._match(only["mesh"][0], only[key][n:]) >= 0).all()           # they sit on the mesh
            grown += int(member[nv0:].sum()) > 0
    assert grown > 0

    cond = mm.stitch_conditioned(dict(res), geom, region_remove="section_points", engine=engine, fill_holes=True,
                                 refine={"passes": 1})
    base = mm.stitch_conditioned(dict(res), geom, region_remove="section_points", engine=engine, fill_holes=True)
    cwant, _, crep2 = mm.refine_mesh(base["mesh"], passes=1, engine=engine)
    assert same_bits(cond["mesh"][0], cwant[0]) and cond["refine_report"] == crep2 and "refine_report" not in base
