"""Mesh relaxation on the device (csrc/mm_relax_kernels.hip, csrc/mm_relax.cpp) against tests/mm_checkers/relax_mesh.py:
vertices and ref_face bit for bit, the integer fields of the report equal, the doubles with equal bits, launches and
bytes as predicted -- over the small solids, tubes one past a workgroup and one past a query block, references of one
chunk and one past it, 0 / 1 / 3 iterations and three factors; a reference that is not the mesh; masks, bands and
borders; messy face lists on both sides; the guard's two cases; the pruning on the long tube; the errors; random small
meshes; and the line label -> remove -> stitch(fill_holes=True, refine=True, relax=True, smooth=True).

The worst cases -- ties across chunks, query blocks flung across the reference, large offsets and scales, degenerate,
thin and NaN seeds, the exact grid -- are in tests/test_gpu_relax_attack.py, with an exact oracle (tests/relax_exact.py)
asked about the device's own output."""
import ctypes as C
import os

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings, strategies as st

from mm_checkers import relax_mesh as RX
from mm_checkers import smooth_mesh as SMO
from test_trim_host import octahedron
from test_smooth_host import tetrahedron
from test_refine_host import same_bits, jitter, wound_tube, open_tube, messy
from test_gpu_stitch import takeoff_case
from test_relax_host import tube_15_17, tube_7_73, long_tube_case

import multimoda_rs_amd as mm
from multimoda_rs_amd import ccta

pytestmark = pytest.mark.gpu

INT_KEYS = ("n_vertices", "n_faces", "n_ref_faces", "n_free", "n_pinned", "n_border", "n_isolated", "iterations_run",
            "n_reverted", "n_flipped_faces")
F64_KEYS = ("initial_distance_sq", "max_displacement_sq", "volume_before", "volume_after")


def bits(x):
    return np.float64(x).view(np.uint64)


def same_relax(mesh, reference, engine, iterations=3, lamb=0.5, pinned=None, want=None):
    """relax_mesh against the checker (want: its answer where the caller has it): (vertices, ref_face, report)."""
    v, f = np.asarray(mesh[0], dtype=np.float64), np.asarray(mesh[1], dtype=np.int64).reshape(-1, 3)
    rv, rf = (None, None) if reference is None else reference
    (gv, gf), face, rep = mm.relax_mesh((v, f), reference, iterations=iterations, lamb=lamb, pinned=pinned, engine=engine)
    wv, wface, wrep = (want or RX.relax(v, f, rv, rf, iterations=iterations, lamb=lamb, pinned=pinned))[:3]
    assert same_bits(gv, wv) and np.array_equal(gf, f)
    assert np.array_equal(face, wface) and face.dtype == np.int64
    for k in INT_KEYS:
        assert rep[k] == wrep[k], k
    for k in F64_KEYS:
        assert bits(rep[k]) == bits(wrep[k]), k
    pred = RX.predict_report(len(v), len(f), wrep["n_ref_faces"], wrep["n_free"], iterations)
    for k in ("n_launches", "bytes_uploaded", "bytes_downloaded"):
        assert rep[k] == pred[k], k
    assert rep["items_run"] + rep["items_skipped"] == pred["items_total"]
    assert 0 <= rep["items_skipped_step0"] <= rep["items_skipped"]
    if iterations == 0:
        assert rep["items_skipped_step0"] == rep["items_skipped"]
    return gv, face, rep


def settled(report):
    """The report without the two counts that depend on the order in which the checked items ran."""
    return {k: x for k, x in report.items() if k not in ("items_run", "items_skipped", "items_skipped_step0")}


def chunk_reference(n_faces):
    """A jittered tube's first n_faces faces: an open strip of the wall with exactly that many reference faces."""
    v, f = wound_tube(12, 14)
    assert len(f) >= n_faces
    return jitter(v, 9), f[:n_faces]


# ---- parity with the checker ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [octahedron, tetrahedron])
@pytest.mark.parametrize("iterations", [0, 1, 3])
def test_small_solids(engine, shape, iterations):
    v, f = shape()
    for lamb in (0.5, 2.0, -0.3):
        same_relax((v, f), None, engine, iterations, lamb)


@pytest.mark.parametrize("tube,n_free", [(tube_15_17, 257), (tube_7_73, 513)])
@pytest.mark.parametrize("iterations,lamb", [(0, 0.5), (1, 0.5), (3, 0.5), (3, 2.0), (3, -0.3)])
def test_tubes_one_past_a_workgroup_and_one_past_a_query_block(engine, tube, n_free, iterations, lamb):
    v, f = tube()
    _, _, rep = same_relax((v, f), None, engine, iterations, lamb)
    assert rep["n_free"] == n_free and rep["n_border"] == 0
    if iterations == 0:
        assert rep["initial_distance_sq"] == 0.0 and rep["max_displacement_sq"] == 0.0


@pytest.mark.parametrize("n_faces", [256, 257])
def test_references_of_one_chunk_and_one_past_it(engine, n_faces):
    rv, rf = chunk_reference(n_faces)
    v, f = tube_15_17()
    _, _, rep = same_relax((0.9 * v, f), (rv, rf), engine, 3, 0.5)
    assert rep["n_ref_faces"] == n_faces and rep["initial_distance_sq"] > 0.0
    assert rep["items_run"] + rep["items_skipped"] == (1 if n_faces == 256 else 2) * 4


# ---- a reference that is not the mesh ------------------------------------------------------------------------------------

def test_smoothed_tube_projected_onto_the_unsmoothed_one_then_relaxed(engine):
    v, f = tube_15_17()
    sv = SMO.smooth(v, f, SMO.taubin_factors(iterations=4))[0]
    (pv, _), face, rep = mm.project_to_mesh((sv, f), (v, f), engine=engine)
    wv, wface, wrep = RX.relax(sv, f, v, f, iterations=0)
    assert same_bits(pv, wv) and np.array_equal(face, wface) and rep["iterations_run"] == 0
    assert rep["initial_distance_sq"] > 0.0 and bits(rep["initial_distance_sq"]) == bits(wrep["initial_distance_sq"])
    assert rep["n_launches"] == RX.predict_report(len(v), len(f), len(f), 257, 0)["n_launches"]
    gv, _, rep2 = same_relax((sv, f), (v, f), engine, 3, 0.5)
    assert bits(rep2["initial_distance_sq"]) == bits(rep["initial_distance_sq"]) and not same_bits(gv, pv)


# ---- masks and borders ---------------------------------------------------------------------------------------------------

def test_pinned_as_mask_and_as_indices_and_a_band(engine):
    v, f = tube_15_17()
    mask = np.zeros(len(v), dtype=bool)
    mask[::3] = True
    a, _, rep = same_relax((v, f), None, engine, 3, 0.5, pinned=mask)
    assert rep["n_pinned"] == int(mask.sum()) and same_bits(a[mask], v[mask])
    (b, _), _, _ = mm.relax_mesh((v, f), iterations=3, pinned=np.flatnonzero(mask), engine=engine)
    assert same_bits(a, b)
    seeds = [0, 1, 2]
    ring = ccta.vertex_rings(f, seeds, 2, len(v), engine=engine)
    (c, _), cface, crep = mm.relax_mesh((v, f), iterations=3, band=(seeds, 2), engine=engine)
    wv, wface, wrep = RX.relax(v, f, iterations=3, pinned=ring < 0)
    assert same_bits(c, wv) and np.array_equal(cface, wface) and crep["n_free"] == wrep["n_free"] == int((ring >= 0).sum())
    assert crep["n_free"] < 60 and crep["bytes_uploaded"] < rep["bytes_uploaded"]      # only free vertices are queries
    both = mm.relax_mesh((v, f), iterations=3, pinned=mask, band=(seeds, 2), engine=engine)[0][0]
    assert same_bits(both, RX.relax(v, f, iterations=3, pinned=mask | (ring < 0))[0])


def test_open_tube_pins_its_rims(engine):
    v, f = open_tube()
    gv, face, rep = same_relax((jitter(v, 7), f), None, engine, 3, 0.5)
    rim = np.r_[0:15, len(v) - 15:len(v)]
    assert rep["n_border"] == 30 and (face[rim] == -1).all() and same_bits(gv[rim], jitter(v, 7)[rim])


def test_messy_faces_as_mesh_and_as_reference(engine):
    v, f = messy()
    for iterations in (0, 2):
        _, _, rep = same_relax((v, f), None, engine, iterations, 0.5)
        assert rep["n_isolated"] == 1 and rep["n_border"] >= 2
    tv, tf = tube_15_17()
    scale = np.abs(tv).max(axis=0)
    same_relax((tv / scale * [1.0, 2.0, 1.0] + [1.0, 0.0, 1.0], tf), (v, f), engine, 2, 0.5)
    # nothing free: every vertex pinned
    _, face, rep = same_relax((tv, tf), None, engine, 2, 0.5, pinned=np.ones(len(tv), dtype=bool))
    assert rep["n_free"] == 0 and (face == -1).all() and rep["n_launches"] == 2 * SMO.volume_launches(len(tf)) + 2
    # no face at all
    (gv, _), face, rep = mm.relax_mesh((tv[:4], np.zeros((0, 3), dtype=np.int64)), engine=engine)
    assert same_bits(gv, tv[:4]) and (face == -1).all() and rep["n_launches"] == 0 and rep["n_isolated"] == 4


# ---- the guard -------------------------------------------------------------------------------------------------------------

def test_guard_cases(engine):
    v, f = octahedron()
    gv, _, rep = same_relax((v, f), None, engine, 3, 1.0)
    assert rep["n_reverted"] == 18 and same_bits(gv, v)
    v, f = tube_15_17()
    _, _, rep = same_relax((v, f), None, engine, 3, 2.0)
    assert rep["n_reverted"] > 0 and rep["n_flipped_faces"] == 0


# ---- pruning ---------------------------------------------------------------------------------------------------------------

def test_long_tube_skips_what_it_must_and_equals_the_unpruned_scan(engine):
    mesh, ref, want, plan, skips = long_tube_case()
    assert len(skips) == 2 and all(n > 0 for n in skips)
    n_b = len(plan["b"])
    (one, _), _, rep = mm.relax_mesh(mesh, ref, iterations=1, lamb=0.5, engine=engine)
    assert same_bits(one, want[3][0]["vertices_after"]) and rep["items_skipped_step0"] <= n_b
    assert rep["items_skipped"] - rep["items_skipped_step0"] >= skips[0]              # the refreshed bounds alone
    _, _, rep = same_relax(mesh, ref, engine, 2, 0.5, want=want)
    later = rep["items_skipped"] - rep["items_skipped_step0"]
    print(f"long tube, 2 iterations: {rep['items_run']} items run; step 0 skipped {rep['items_skipped_step0']} of its "
          f"{n_b} checked items, the iterations {later} of {2 * (n_b + len(plan['a']))}, must skip {skips}")
    assert rep["items_skipped_step0"] <= n_b and later >= sum(skips)


# ---- errors ----------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_outputs_untouched(engine):
    N = mm._native
    L = N.lib()
    v, f = octahedron()
    f = np.ascontiguousarray(f, dtype=np.int64)
    with pytest.raises(ValueError, match="out of range"):
        mm.relax_mesh((v, [[0, 1, 6]]), engine=engine)
    with pytest.raises(ValueError, match="negative"):
        mm.relax_mesh((v, f), iterations=-1, engine=engine)
    with pytest.raises(ValueError, match="finite"):
        mm.relax_mesh((v, f), lamb=float("nan"), engine=engine)
    with pytest.raises(ValueError, match="non-finite"):
        mm.relax_mesh((np.where(v > 0, np.inf, v), f), engine=engine)
    with pytest.raises(ValueError, match="one entry per vertex"):
        mm.relax_mesh((v, f), pinned=np.zeros(5, dtype=bool), engine=engine)
    with pytest.raises(RuntimeError, match="no reference face"):
        mm.relax_mesh((v, f), (v, np.zeros((0, 3), dtype=np.int64)), engine=engine)
    out, face, rep = np.full((6, 3), 7.0), np.full(6, 7, dtype=np.int64), N.MMRelaxReport()
    bad_f, bad_v = f.copy(), v.copy()
    bad_f[3, 1] = 6
    bad_v[2, 1] = np.nan
    none = np.zeros((0, 3), dtype=np.int64)

    def call(vv=v, ff=f, rv=None, rf=None, rnf=0, it=1, lam=0.5, report=C.byref(rep)):
        return L.mm_mesh_relax(engine.handle, N._ptr(vv), 6, N._ptr(ff), 8, N._ptr(rv), 0 if rv is None else 6, N._ptr(rf),
                               rnf, None, it, lam, N._ptr(out), N._ptr(face), report)

    assert call(vv=bad_v) == -2 and call(ff=bad_f) == -2 and call(it=-1) == -2 and call(lam=float("inf")) == -2
    assert call(report=None) == -2 and call(rv=v, rf=none, rnf=0) == -2 and call(rv=bad_v, rf=f, rnf=8) == -2
    assert call(rv=v, rf=bad_f, rnf=8) == -2
    assert (out == 7.0).all() and (face == 7).all()
    assert call() == 0 and rep.n_free == 6 and (face >= 0).all()


# ---- random small meshes -----------------------------------------------------------------------------------------------------

@settings(max_examples=30 * int(os.environ.get("MM_HYP_SCALE", "1")), deadline=None, derandomize=True, database=None,
          suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(seed=st.integers(0, 2**31 - 1), n_around=st.integers(3, 9), n_rings=st.integers(2, 6), iterations=st.integers(0, 3),
       lamb=st.sampled_from([0.5, 1.0, 2.0, -0.3, 0.0]), pin=st.sampled_from([None, 0.2, 1.0]),
       own=st.booleans(), extra=st.integers(0, 6))
def test_random_small_meshes(engine, seed, n_around, n_rings, iterations, lamb, pin, own, extra):
    r = np.random.default_rng(seed)
    v, f = wound_tube(n_around, n_rings)
    v = v + 0.05 * r.standard_normal(v.shape)
    f = np.concatenate([f, r.integers(0, len(v), (extra, 3))])            # repeated corners, extra owners, crossings
    pinned = None if pin is None else r.random(len(v)) < pin
    ref = None
    if not own:
        rv, rf = wound_tube(int(r.integers(3, 8)), int(r.integers(2, 5)))
        ref = (rv * r.uniform(0.5, 1.5) + 0.02 * r.standard_normal(rv.shape), rf)
    same_relax((v, f), ref, engine, iterations, lamb, pinned)


# ---- the line label -> remove -> stitch -----------------------------------------------------------------------------------

def test_stitch_with_and_without_relaxation(engine):
    res, geom, frames = takeoff_case(engine)
    kw = dict(region_remove="section_points", engine=engine, fill_holes=True, refine=True)
    plain = mm.stitch(dict(res), geom, **kw)
    again = mm.stitch(dict(res), geom, relax=False, **kw)
    assert "relax_report" not in plain and sorted(plain) == sorted(again)
    assert same_bits(plain["mesh"][0], again["mesh"][0]) and np.array_equal(plain["mesh"][1], again["mesh"][1])
    want, _, wrep = mm.relax_mesh(plain["mesh"], engine=engine)
    only = mm.stitch(dict(res), geom, relax=True, **kw)
    assert same_bits(only["mesh"][0], want[0]) and np.array_equal(only["mesh"][1], plain["mesh"][1])
    assert settled(only["relax_report"]) == settled(wrep) and wrep["n_free"] > 0 and wrep["iterations_run"] == 5
    two = mm.stitch(dict(res), geom, relax={"iterations": 2}, **kw)
    assert two["relax_report"]["iterations_run"] == 2 and not same_bits(two["mesh"][0], want[0])
    assert not same_bits(want[0], plain["mesh"][0])
    synced = 0
    for key in ccta.SYNC_KEYS:                                            # the lists follow their vertices
        if key in plain and len(plain[key]):
            at = ccta._match(plain["mesh"][0], plain[key])
            assert same_bits(only[key], want[0][at[at >= 0]])
            synced += 1
    assert synced > 0
    full = mm.stitch(dict(res), geom, relax=True, smooth=True, **kw)
    smoothed, srep = mm.smooth_mesh(want, engine=engine)
    assert same_bits(full["mesh"][0], smoothed[0]) and full["smooth_report"] == srep and settled(full["relax_report"]) == settled(wrep)
    assert "refine_report" in full and "fill_report" in full
