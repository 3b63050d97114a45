"""Every engine-taking function of include/mm_ccta.h that accepts `faces` rejects an out-of-range face index the same
way: MM_ERR_INVALID, "<function name>: face index out of range", and nothing written to the output arrays.  The mesh is
two triangles on 4 vertices whose last index is nv (2^31 for mm_fix_winding, which has no nv and bounds the index by
what an int32 holds).  Every other argument is valid, so the face check is the one that fires.

Four functions clear one output in front of the face check (the order of the checks is part of the ABI's behaviour):
mm_mesh_assemble and mm_condition_rims their report, mm_mesh_split_rim_edges its info, mm_faces_near_points its
selection.  Those are zero afterwards; every other output keeps its fill.  With a NULL engine every function returns
MM_ERR_INVALID with "engine == NULL" in front of every other check, and writes nothing at all."""
import ctypes as C

import numpy as np
import pytest

import multimoda_rs_amd as mm

pytestmark = pytest.mark.gpu

N = mm._native
MM_ERR_INVALID = -2
NV, NF = 4, 2
VERTS = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0]])


def _i64(n, fill=-77):
    return np.full(n, fill, dtype=np.int64)


def _f64(n):
    return np.full(n, 7.5, dtype=np.float64)


def _i32(n):
    return np.full(n, -77, dtype=np.int32)


def _u8(n):
    return np.full(n, 0xA5, dtype=np.uint8)


def _struct(cls):
    """A report filled with 0x5A bytes, and the byte view that watches it."""
    s = cls()
    C.memset(C.byref(s), 0x5A, C.sizeof(s))
    return s, np.frombuffer(s, dtype=np.uint8)


# Each builder returns (arguments behind the engine, {name: output array}, names the function clears before the check).
def _open_boundary_edges(f):
    out = {"edges": _i64(6 * NF)}
    return [N._ptr(f), NF, NV, N._ptr(out["edges"])], out, ()


def _clean_open_boundary(f):
    out = {"drop": _i64(NV), "ring_len": _i64(NV), "ring_idx": _i64(NV), "counts": _i64(3)}
    return [N._ptr(f), NF, N._ptr(VERTS), NV, None, 0, -1, 0.5, 3, N._ptr(out["drop"]), N._ptr(out["ring_len"]),
            N._ptr(out["ring_idx"]), N._ptr(out["counts"])], out, ()


def _trim_mesh(f):
    region = np.zeros(NV, dtype=np.uint8)
    out = {"out_vertices": _f64(3 * NV), "out_faces": _i64(3 * NF), "ring_len": _i64(NV), "ring_idx": _i64(NV),
           "counts": _i64(4)}
    return [N._ptr(VERTS), NV, N._ptr(f), NF, N._ptr(region), 0, -1, 0.5, 3, N._ptr(out["out_vertices"]),
            N._ptr(out["out_faces"]), N._ptr(out["ring_len"]), N._ptr(out["ring_idx"]), N._ptr(out["counts"]), region], out, ()


def _fix_winding(f):
    out = {"out_faces": _i64(3 * NF), "info": _i64(3)}
    return [N._ptr(f), NF, N._ptr(out["out_faces"]), N._ptr(out["info"])], out, ()


def _mesh_assemble(f):
    vert_off, face_off = np.array([0, NV], dtype=np.int64), np.array([0, NF], dtype=np.int64)
    rep, view = _struct(N.MMAssembleReport)
    out = {"out_vertices": _f64(3 * NV), "out_faces": _i64(3 * NF), "report": view}
    return [1, N._ptr(VERTS), N._ptr(vert_off), N._ptr(f), N._ptr(face_off), 3, 1, 1, N._ptr(out["out_vertices"]),
            N._ptr(out["out_faces"]), C.byref(rep), vert_off, face_off, rep], out, ("report",)


def _fill_holes(f):
    rep, view = _struct(N.MMFillReport)
    out = {"out_vertices": _f64(3 * (NV + 4)), "out_faces": _i64(3 * (NF + 8)), "report": view}
    return [N._ptr(VERTS), NV, N._ptr(f), NF, 1, NV + 4, NF + 8, N._ptr(out["out_vertices"]), N._ptr(out["out_faces"]),
            C.byref(rep), rep], out, ()


def _smooth_labels_faces(f):
    labels = np.array([0, 1, 0, 1], dtype=np.uint8)
    out = {"out_labels": _u8(NV), "info": _i64(4)}
    return [N._ptr(labels), NV, N._ptr(f), NF, 1, N._ptr(out["out_labels"]), N._ptr(out["info"]), labels], out, ()


def _mesh_adjacency_csr(f):
    out = {"off": _i64(NV + 1), "nb": _i64(6 * NF), "info": _i64(4)}
    return [N._ptr(f), NF, NV, 6 * NF, N._ptr(out["off"]), N._ptr(out["nb"]), N._ptr(out["info"])], out, ()


def _mesh_smooth(f):
    factors = np.array([0.5], dtype=np.float64)
    rep, view = _struct(N.MMSmoothReport)
    out = {"out_vertices": _f64(3 * NV), "report": view}
    return [N._ptr(VERTS), NV, N._ptr(f), NF, N._ptr(factors), 1, None, N._ptr(out["out_vertices"]), C.byref(rep),
            factors, rep], out, ()


def _mesh_vertex_rings(f):
    seeds = np.array([0], dtype=np.int64)
    out = {"ring_out": _i32(NV), "info": _i64(3)}
    return [N._ptr(f), NF, NV, N._ptr(seeds), 1, 2, N._ptr(out["ring_out"]), N._ptr(out["info"]), seeds], out, ()


def _mesh_layer_push(f):
    seeds = np.array([0], dtype=np.int64)
    origin, normal = np.zeros(3), np.array([0.0, 0.0, 1.0])
    out = {"out_vertices": _f64(3 * NV), "out_layer": _i32(NV), "info": _i64(3)}
    return [N._ptr(VERTS), NV, N._ptr(f), NF, N._ptr(seeds), 1, N._ptr(origin), N._ptr(normal), 0.1, 2,
            N._ptr(out["out_vertices"]), N._ptr(out["out_layer"]), N._ptr(out["info"]), seeds, origin, normal], out, ()


def _mesh_split_rim_edges(f):
    ring, counts = np.array([0, 1, 2], dtype=np.int64), np.array([1, 0, 0], dtype=np.int64)
    out = {"out_vertices": _f64(3 * (NV + 4)), "out_faces": _i64(3 * (NF + 8)), "out_ring_idx": _i64(8), "info": _i64(6)}
    return [N._ptr(VERTS), NV, N._ptr(f), NF, N._ptr(ring), 3, N._ptr(counts), NV + 4, NF + 8, N._ptr(out["out_vertices"]),
            N._ptr(out["out_faces"]), N._ptr(out["out_ring_idx"]), N._ptr(out["info"]), ring, counts], out, ("info",)


def _condition_rims(f):
    centroid = np.zeros(3)
    par = N.MMRimParams()
    par.vert_cap, par.face_cap, par.ring_cap = NV + 4, NF + 8, 8
    par.smooth_alpha, par.angle_threshold_deg, par.clamp_overshoot, par.layer_step_mm = 0.5, 30.0, 0.1, 0.1
    rep, view = _struct(N.MMRimReport)
    out = {"out_vertices": _f64(3 * (NV + 4)), "out_faces": _i64(3 * (NF + 8)), "out_prox": _f64(24), "out_dist": _f64(24),
           "report": view}
    return [N._ptr(VERTS), NV, N._ptr(f), NF, None, 0, None, 0, None, 0, N._ptr(centroid), None, None, 0, C.byref(par),
            N._ptr(out["out_vertices"]), N._ptr(out["out_faces"]), N._ptr(out["out_prox"]), N._ptr(out["out_dist"]),
            C.byref(rep), centroid, par, rep], out, ("report",)


def _faces_near_points(f):
    pts = np.array([[0.5, 0.5, 0.0]])
    out = {"face_selected": _u8(NF)}
    return [N._ptr(VERTS), NV, N._ptr(f), NF, N._ptr(pts), 1, 0.25, N._ptr(out["face_selected"]), pts], out, ("face_selected",)


# name -> (builder, ctypes arguments the C function takes behind the engine; what follows them only keeps arrays alive)
CASES = {
    "mm_open_boundary_edges": (_open_boundary_edges, 4),
    "mm_clean_open_boundary": (_clean_open_boundary, 13),
    "mm_trim_mesh": (_trim_mesh, 14),
    "mm_fix_winding": (_fix_winding, 4),
    "mm_mesh_assemble": (_mesh_assemble, 11),
    "mm_fill_holes": (_fill_holes, 10),
    "mm_smooth_labels_faces": (_smooth_labels_faces, 7),
    "mm_mesh_adjacency_csr": (_mesh_adjacency_csr, 7),
    "mm_mesh_smooth": (_mesh_smooth, 9),
    "mm_mesh_vertex_rings": (_mesh_vertex_rings, 8),
    "mm_mesh_layer_push": (_mesh_layer_push, 13),
    "mm_mesh_split_rim_edges": (_mesh_split_rim_edges, 13),
    "mm_condition_rims": (_condition_rims, 20),
    "mm_faces_near_points": (_faces_near_points, 8),
}


def _bad_faces(name):
    last = 2 ** 31 if name == "mm_fix_winding" else NV
    return np.array([[0, 1, 2], [0, 2, last]], dtype=np.int64)


def _call(name, handle):
    build, n_args = CASES[name]
    faces = _bad_faces(name)
    args, out, cleared = build(faces)
    before = {k: a.copy() for k, a in out.items()}
    rc = getattr(N.lib(), name)(handle, *args[:n_args])
    return rc, N.last_error(), out, before, cleared


def test_every_ccta_function_with_faces_is_covered():
    """The header's own list: an entry point added to include/mm_ccta.h with an engine and faces must get a case here."""
    import os
    import re
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mm_ccta.h")
    with open(header) as fh:
        text = fh.read()
    found = {m.group(1) for m in re.finditer(r"\b(mm_\w+)\(mm_engine\*[^;]*\bconst int64_t\* faces\b[^;]*;", text)}
    assert found == set(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_face_index_out_of_range(engine, name):
    rc, err, out, before, cleared = _call(name, engine.handle)
    assert rc == MM_ERR_INVALID
    assert err == name + ": face index out of range"
    for k, a in out.items():
        if k in cleared:
            assert not a.any(), k
        else:
            assert np.array_equal(a, before[k]), k


@pytest.mark.parametrize("name", sorted(CASES))
def test_null_engine(name):
    rc, err, out, before, _ = _call(name, None)
    assert rc == MM_ERR_INVALID
    assert err == "engine == NULL"
    for k, a in out.items():
        assert np.array_equal(a, before[k]), k
