"""Mesh edge collapse on the device (csrc/mm_collapse_kernels.hip, csrc/mm_collapse.cpp) against the checker
(tests/mm_checkers/collapse_edges.py): the vertices bit for bit, identical faces, origin and target, every integer field
of the report equal -- the collapses and candidates per pass, the blocked counts, the short edges, the launch and byte
counts -- with bit-equal volumes.  Shapes: the small solids, a mesh one vertex past a workgroup (257), its jittered form
refined and collapsed at 0.6 (dozens of passes, the compaction, chains in target), the refined open tube, a messy face
list and an empty one, one hand-built shape per guard, 0 / 1 / 2 passes, a mask as booleans, as indices and a band,
shuffled faces, the same call twice, random meshes with arbitrary indices, the argument checks, the line label -> remove
-> stitch(..., collapse=True), and isotropic_remesh against the four public calls."""
import ctypes as C
import os

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings, strategies as st

from mm_checkers import collapse_edges as CE
from mm_checkers import stitch_mesh as SM
from test_refine_host import same_bits
from test_flip_host import refined_tube
from test_collapse_host import SHAPES, collapsed
from test_gpu_refine import bits_equal
from test_gpu_stitch import takeoff_case

import multimoda_rs_amd as mm
from multimoda_rs_amd import ccta

pytestmark = pytest.mark.gpu

N = mm._native
MM_ERR_INVALID = -2
INT_KEYS = tuple(k for k in ccta.COLLAPSE_REPORT_KEYS if not k.startswith("volume")) + ("collapses_per_pass", "candidates_per_pass")


def same_collapse(v, f, L, engine, want=None, **kw):
    (gv, gf), origin, target, rep = mm.collapse_edges((v, f), L, engine=engine, **kw)
    if want is None:
        mask = ccta._pin_mask(kw.get("pinned"), kw.get("band"), ccta._p3(v), ccta._faces3(f), engine)
        want = CE.collapse(v, f, L, mask=mask, min_ratio=kw.get("min_ratio", CE.MIN_RATIO), max_ratio=kw.get("max_ratio", CE.MAX_RATIO),
                           crease_cos=CE.crease_cos(kw.get("crease_deg", 30.0)), quality_keep=kw.get("quality_keep", 0.5),
                           max_passes=kw.get("passes", 50))
    wv, wf, worigin, wtarget, wrep = want[:5]
    assert gf.dtype == np.int64 and origin.dtype == np.int64 and target.dtype == np.int64
    assert same_bits(gv, wv) and np.array_equal(gf, wf) and np.array_equal(origin, worigin) and np.array_equal(target, wtarget)
    for k in INT_KEYS:
        assert rep[k] == wrep[k], (k, rep[k], wrep[k])
    for k in ("volume_before", "volume_after"):
        assert bits_equal(rep[k], wrep[k]), (k, rep[k], wrep[k])
    return (gv, gf, origin, target), rep


def same_shape(name, engine, **kw):
    fn, L, mask = SHAPES[name]
    v, f = fn()
    return same_collapse(np.asarray(v, dtype=np.float64), np.asarray(f, dtype=np.int64), L, engine, want=collapsed(name)[2:7],
                         pinned=mask, **kw)


@pytest.mark.parametrize("name", ["tetrahedron", "octahedron"])
def test_small_solids_stay_whole(engine, name):
    out, rep = same_shape(name, engine)
    assert rep["n_collapses"] == 0 and rep["converged"] == 1 and rep["passes_run"] == 1
    assert rep["n_launches"] == 10 + 9 + 2 * 2 and rep["bytes_downloaded"] == 28 * len(out[0]) + 12 * len(out[1]) + 4 * len(out[0]) + 128


def test_one_vertex_past_a_workgroup(engine):
    out, rep = same_shape("tube", engine)
    assert rep["n_vertices"] == 257 and rep["n_collapses"] == 50 and rep["converged"] == 0   # equal lengths: one a pass


def test_refined_tube_takes_dozens_of_passes(engine):
    v, f = refined_tube()
    want = collapsed("refined_tube")
    out, rep = same_shape("refined_tube", engine)
    assert rep["passes_run"] >= 24 and rep["n_collapses"] > 500 and rep["converged"] == 1
    assert rep["collapses_per_pass"][:15] == [len(p["collapsed"]) for p in want[7][:15]]
    assert (out[3] != np.arange(len(v))).sum() > rep["n_collapses"]       # target renumbers the survivors too
    _, n_open, n_nonmanifold = SM.face_adjacency(out[1])
    assert n_open == 0 and n_nonmanifold == 0
    # the same call twice: the same bits
    again, origin, target, rep2 = mm.collapse_edges((v, f), 0.6, engine=engine)
    assert same_bits(again[0], out[0]) and np.array_equal(again[1], out[1]) and np.array_equal(target, out[3]) and rep2 == rep


def test_refined_open_tube(engine):
    _, rep = same_shape("refined_open_tube", engine)
    assert rep["n_open_edges"] > 0 and rep["n_collapses"] > 0 and rep["blocked_fixed"] > 0


def test_messy_face_list_and_no_faces(engine):
    _, rep = same_shape("messy", engine)
    assert rep["n_nonmanifold_edges"] == 1 and rep["n_open_edges"] > 0 and rep["blocked_fixed"] == 9
    v = SHAPES["messy"][0]()[0]
    empty = np.zeros((0, 3), dtype=np.int64)
    out, rep = same_collapse(v, empty, 1.0, engine)
    assert rep["n_launches"] == 0 and out[1].shape == (0, 3) and np.array_equal(out[2], np.arange(len(v)))


@pytest.mark.parametrize("name, blocked", [("patch", None), ("link", "blocked_link"), ("long", "blocked_long"),
                                           ("fold", "blocked_normal"), ("needle", "blocked_quality")])
def test_each_guard_on_its_shape(engine, name, blocked):
    _, rep = same_shape(name, engine)
    assert rep["n_collapses"] == 1 if blocked is None else rep[blocked] > 0


@pytest.mark.parametrize("passes", [0, 1, 2])
def test_pass_counts(engine, passes):
    v, f = refined_tube()
    out, rep = same_collapse(v, f, 0.6, engine, passes=passes)
    assert rep["passes_run"] == passes and rep["converged"] == 0
    if passes == 0:
        assert np.array_equal(out[1], f) and same_bits(out[0], v) and rep["n_short_after"] == rep["n_short_before"] > 0


def test_pinned_as_mask_and_as_indices_and_a_band(engine):
    v, f = refined_tube()
    mask = np.zeros(len(v), dtype=bool)
    mask[::3] = True
    a, rep = same_collapse(v, f, 0.6, engine, pinned=mask, passes=4)
    assert rep["n_collapses"] > 0 and rep["bytes_uploaded"] == 25 * len(v) + 12 * len(f) and np.isin(np.flatnonzero(mask), a[2]).all()
    b = mm.collapse_edges((v, f), 0.6, pinned=np.flatnonzero(mask), passes=4, engine=engine)
    assert np.array_equal(b[0][1], a[1]) and np.array_equal(b[1], a[2])
    out, rep = same_collapse(v, f, 0.6, engine, band=([700], 3), passes=4)
    ring = mm.vertex_rings(f, [700], 3, len(v), engine)
    gone = np.setdiff1d(np.arange(len(v)), out[2])
    assert len(gone) > 0 and (ring[gone] >= 0).all()
    same_collapse(v, f, 0.6, engine, pinned=mask, band=([700], 5), crease_deg=60.0, quality_keep=0.25, min_ratio=0.7,
                  max_ratio=1.5, passes=4)


def test_shuffled_faces_change_the_result_and_still_equal_the_checker(engine):
    v, f = refined_tube()
    r = np.random.default_rng(5)
    g = f[r.permutation(len(f))]
    g = np.stack([np.roll(t, int(k)) for t, k in zip(g, r.integers(0, 3, len(g)))])
    other, rep = same_collapse(v, g, 0.6, engine, passes=6)
    base = CE.collapse(v, f, 0.6, max_passes=6)
    assert rep["n_collapses"] > 100 and not np.array_equal(other[2], base[2])


@settings(max_examples=40 * int(os.environ.get("MM_HYP_SCALE", "1")), deadline=None, derandomize=True, database=None,
          suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(seed=st.integers(0, 2**31 - 1), nv=st.integers(1, 12), nf=st.integers(0, 24), passes=st.integers(0, 4),
       pin=st.sampled_from([None, 0.2]), crease=st.sampled_from([30.0, 90.0]), keep=st.sampled_from([0.0, 0.5]),
       L=st.sampled_from([1.0, 4.0, 100.0]))
def test_random_small_meshes(engine, seed, nv, nf, passes, pin, crease, keep, L):
    r = np.random.default_rng(seed)
    v = r.uniform(-3, 3, (nv, 3))
    f = r.integers(0, nv, (nf, 3))
    pinned = None if pin is None else r.random(nv) < pin
    same_collapse(v, f, L, engine, passes=passes, pinned=pinned, crease_deg=crease, quality_keep=keep)


def test_face_index_out_of_range_null_engine_and_bad_numbers(engine):
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0]])
    bad = np.array([[0, 1, 2], [0, 2, 4]], dtype=np.int64)
    good = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int64)

    def raw(handle, f, L=1.0, lo=0.8, hi=4.0 / 3.0, crease_cos=0.5, keep=0.5, passes=3):
        ov, of = np.full((4, 3), -77.0), np.full((2, 3), -77, dtype=np.int64)
        origin, target = np.full(4, -77, dtype=np.int64), np.full(4, -77, dtype=np.int64)
        rep = N.MMCollapseReport()
        C.memset(C.byref(rep), 0x5A, C.sizeof(rep))
        rc = N.lib().mm_mesh_collapse_edges(handle, N._ptr(v), 4, N._ptr(f), 2, None, L, lo, hi, crease_cos, keep, passes,
                                            N._ptr(ov), N._ptr(of), N._ptr(origin), N._ptr(target), C.byref(rep))
        return rc, ((ov == -77).all() and (of == -77).all() and (origin == -77).all() and (target == -77).all() and
                    (np.frombuffer(rep, dtype=np.uint8) == 0x5A).all())

    for handle, err in ((engine.handle, "mm_mesh_collapse_edges: face index out of range"), (None, "engine == NULL")):
        rc, untouched = raw(handle, bad)
        assert rc == MM_ERR_INVALID and N.last_error() == err and untouched
    nan, inf = float("nan"), float("inf")
    for kw in (dict(crease_cos=-0.1), dict(crease_cos=1.1), dict(crease_cos=nan), dict(keep=-0.1), dict(keep=1.1), dict(keep=nan),
               dict(passes=-1), dict(L=0.0), dict(L=-1.0), dict(L=nan), dict(L=inf), dict(lo=0.0), dict(lo=1.1), dict(lo=nan),
               dict(hi=0.9), dict(hi=nan), dict(hi=inf)):
        rc, untouched = raw(engine.handle, good, **kw)
        assert rc == MM_ERR_INVALID and untouched, kw
    assert raw(engine.handle, good)[0] == 0


# ---- the line label -> remove -> stitch -----------------------------------------------------------------------------------

def test_stitch_with_and_without_collapse(engine):
    res, geom, frames = takeoff_case(engine)
    kw = dict(region_remove="section_points", engine=engine, fill_holes=True, refine=True)
    base = mm.stitch(dict(res), geom, **kw)                               # refined: what the collapse sees
    again = mm.stitch(dict(res), geom, collapse=False, **kw)
    assert "collapse_report" not in base and sorted(base) == sorted(again)
    assert same_bits(base["mesh"][0], again["mesh"][0]) and np.array_equal(base["mesh"][1], again["mesh"][1])
    assert all(same_bits(base[k], again[k]) for k in ccta.SYNC_KEYS if base.get(k) is not None and len(base[k]))

    v, f = base["mesh"]
    iv = ccta._match(v, base["anomalous_points"])
    iv = np.unique(iv[iv >= 0])
    assert len(iv) > 0
    want, origin, target, wrep = mm.collapse_edges(base["mesh"], pinned=iv, engine=engine)
    assert wrep["n_collapses"] > 0 and wrep["n_vertices_out"] == len(v) - wrep["n_collapses"]
    full = mm.stitch(dict(res), geom, collapse=True, **kw)
    assert full["collapse_report"] == wrep and "refine_report" in full
    assert same_bits(full["mesh"][0], want[0]) and np.array_equal(full["mesh"][1], want[1])
    _, n_open, n_nonmanifold = SM.face_adjacency(full["mesh"][1])
    assert n_open == 0 and n_nonmanifold == 0                             # still watertight
    lumen = np.isin(f, iv).all(axis=1)
    kept = target[f[lumen]]
    assert lumen.sum() > 0 and np.isin(iv, origin).all()
    rows = {tuple(t) for t in full["mesh"][1].tolist()}
    assert all(tuple(t) in rows for t in kept.tolist())                   # the IV lumen's faces as they were
    gone = v[np.setdiff1d(np.arange(len(v)), origin)]
    for k in ccta.SYNC_KEYS:                                              # a removed vertex leaves the point lists
        if full.get(k) is not None and len(full[k]):
            assert (ccta._match(gone, full[k]) < 0).all() and len(full[k]) <= len(base[k])
    two = mm.stitch_conditioned(dict(res), geom, region_remove="section_points", engine=engine, fill_holes=True, refine=True,
                                collapse={"passes": 2}, flip=True)
    assert 1 <= two["collapse_report"]["passes_run"] <= 2 and two["collapse_report"]["n_collapses"] > 0
    assert two["flip_report"]["n_vertices"] == two["collapse_report"]["n_vertices_out"]     # the flips ran behind it


def test_isotropic_remesh_is_the_four_calls(engine):
    v, f = refined_tube()
    L = 0.5
    mask = np.zeros(len(v), dtype=bool)
    mask[::7] = True
    (gv, gf), rep = mm.isotropic_remesh((v, f), L, iterations=2, pinned=mask, relax={"iterations": 2}, engine=engine)
    cur, m = (v, f), mask
    for it in range(2):
        cur, parents, r0 = mm.refine_mesh(cur, L, passes=1, engine=engine)
        m = np.concatenate([m, np.zeros(len(parents), dtype=bool)])
        cur, origin, _, r1 = mm.collapse_edges(cur, L, pinned=m, engine=engine)
        m = m[origin]
        cur, r2 = mm.flip_edges(cur, pinned=m, engine=engine)
        cur, _, r3 = mm.relax_mesh(cur, (v, f), iterations=2, pinned=m, engine=engine)
        assert rep["iterations"][it] == {"refine": r0, "collapse": r1, "flip": r2, "relax": r3}
    assert same_bits(gv, cur[0]) and np.array_equal(gf, cur[1]) and len(rep["iterations"]) == 2
    assert rep["iterations"][0]["collapse"]["n_collapses"] > 0
    assert 0.0 <= rep["share_in_range_before"] <= 1.0 and 0.0 <= rep["share_in_range_after"] <= 1.0
    assert (rep["n_vertices_after"], rep["n_faces_after"]) == (len(gv), len(gf))
    pinned_pts = v[mask]
    assert (ccta._match(gv, pinned_pts) >= 0).all()                       # no pinned vertex vanished or moved
