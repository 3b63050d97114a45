"""Mesh edge flips on the device (csrc/mm_flip_kernels.hip, csrc/mm_flip.cpp) against the checker
(tests/mm_checkers/flip_edges.py): identical faces and every field of the report equal -- the flips and candidates per
pass, the blocked counts, the deviations, the launch and byte counts -- with bit-equal volumes.  Shapes: the small solids,
a mesh one vertex past a workgroup (257), its jittered form (the cap centres serialise), that form refined (a dozen
passes), the refined open tube, a messy face list, the hand-built existing-edge shape, 0 / 1 / 2 passes, a mask and a
band, shuffled faces, the same call twice, random meshes with arbitrary indices, the valences, the argument checks, and
the line label -> remove -> stitch(fill_holes=True, refine=True, flip=True, relax=True)."""
import ctypes as C
import os

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings, strategies as st

from mm_checkers import flip_edges as FE
from mm_checkers import smooth_mesh as SMO
from mm_checkers import stitch_mesh as SM
from test_trim_host import octahedron
from test_smooth_host import tetrahedron
from test_refine_host import same_bits, messy
from test_flip_host import (flipped, tube, jittered_tube, refined_tube, refined_open_tube, existing_edge_shape)
from test_gpu_refine import bits_equal
from test_gpu_stitch import takeoff_case

import multimoda_rs_amd as mm
from multimoda_rs_amd import ccta

pytestmark = pytest.mark.gpu

N = mm._native
MM_ERR_INVALID = -2
INT_KEYS = tuple(k for k in ccta.FLIP_REPORT_KEYS if not k.startswith("volume")) + ("flips_per_pass", "candidates_per_pass")


def same_flip(v, f, engine, want=None, **kw):
    (gv, gf), rep = mm.flip_edges((v, f), engine=engine, **kw)
    if want is None:
        mask = ccta._pin_mask(kw.get("pinned"), kw.get("band"), ccta._p3(v), ccta._faces3(f), engine)
        want = FE.flip(v, f, mask=mask, crease_cos=FE.crease_cos(kw.get("crease_deg", 30.0)),
                       quality_keep=kw.get("quality_keep", 0.5), max_passes=kw.get("passes", 50))
    wf, wrep = want[:2]
    assert gf.dtype == np.int64 and np.array_equal(gf, wf) and same_bits(gv, v)
    for k in INT_KEYS:
        assert rep[k] == wrep[k], (k, rep[k], wrep[k])
    for k in ("volume_before", "volume_after"):
        assert bits_equal(rep[k], wrep[k]), (k, rep[k], wrep[k])
    return gf, rep


@pytest.mark.parametrize("solid", [tetrahedron, octahedron])
def test_small_solids_flip_nothing(engine, solid):
    v, f = solid()
    out, rep = same_flip(v, f, engine)
    assert rep["n_flips"] == 0 and rep["converged"] == 1 and rep["passes_run"] == 1 and np.array_equal(out, f)
    assert rep["n_launches"] == 5 + 2 * 2 and rep["bytes_downloaded"] == 12 * len(f) + 128


def test_one_vertex_past_a_workgroup(engine):
    v, f = tube()
    assert len(v) == 257
    _, rep = same_flip(v, f, engine, want=flipped("tube")[2:4])
    assert rep["n_flips"] == 0 and rep["blocked_quality"] > 0


def test_cap_centres_serialise(engine):
    v, f = jittered_tube()
    _, rep = same_flip(v, f, engine, want=flipped("jittered_tube")[2:4])
    assert rep["passes_run"] > 2 and rep["n_flips"] > 2


def test_refined_tube_takes_a_dozen_passes(engine):
    v, f = refined_tube()
    want = flipped("refined_tube")
    out, rep = same_flip(v, f, engine, want=want[2:4])
    assert rep["passes_run"] >= 10 and rep["n_flips"] > 300 and rep["converged"] == 1
    assert rep["flips_per_pass"] == [len(p["flipped"]) for p in want[4]] + [0] * (16 - len(want[4]))
    assert rep["deviation_after"] == rep["deviation_before"] - sum(k["g"] for p in want[4] for k in p["flipped"])
    _, n_open, n_nonmanifold = SM.face_adjacency(out)
    assert n_open == 0 and n_nonmanifold == 0
    # the same call twice: the same bits
    again, rep2 = mm.flip_edges((v, f), engine=engine)
    assert np.array_equal(again[1], out) and rep2 == rep


def test_refined_open_tube(engine):
    v, f = refined_open_tube()
    _, rep = same_flip(v, f, engine, want=flipped("refined_open_tube")[2:4])
    assert rep["n_open_edges"] > 0 and rep["n_flips"] > 0


def test_messy_face_list_and_no_faces(engine):
    v, f = messy()
    _, rep = same_flip(v, f, engine)
    assert rep["n_nonmanifold_edges"] == 1 and rep["n_open_edges"] > 0
    empty = np.zeros((0, 3), dtype=np.int64)
    out, rep = same_flip(v, empty, engine)
    assert rep["n_launches"] == 0 and out.shape == (0, 3) and rep["deviation_after"] == 36 * len(v)


def test_the_existing_edge_blocks(engine):
    v, f = existing_edge_shape()
    out, rep = same_flip(v, f, engine, want=flipped("existing_edge")[2:4])
    assert rep["blocked_existing"] > 0 and (np.sort(out, axis=1) == [0, 1, 2]).all(axis=1).any()


@pytest.mark.parametrize("passes", [0, 1, 2])
def test_pass_counts(engine, passes):
    v, f = refined_tube()
    out, rep = same_flip(v, f, engine, passes=passes)
    assert rep["passes_run"] == passes and rep["converged"] == 0
    assert rep["n_launches"] == 5 * passes + 3 + 2 * SMO.volume_launches(len(f))
    if passes == 0:
        assert np.array_equal(out, f) and rep["deviation_after"] == rep["deviation_before"] == 5656 and rep["n_edges"] == 4374


def test_pinned_as_mask_and_as_indices_and_a_band(engine):
    v, f = refined_tube()
    mask = np.zeros(len(v), dtype=bool)
    mask[::3] = True
    a, rep = same_flip(v, f, engine, pinned=mask)
    assert rep["n_masked_edges"] > 0 and rep["n_flips"] > 0 and rep["bytes_uploaded"] == 25 * len(v) + 12 * len(f)
    b, _ = mm.flip_edges((v, f), pinned=np.flatnonzero(mask), engine=engine)
    assert np.array_equal(b[1], a) and not np.array_equal(a, flipped("refined_tube")[2])
    out, rep = same_flip(v, f, engine, band=([700], 3))
    ring = mm.vertex_rings(f, [700], 3, len(v), engine)
    changed = np.flatnonzero((out != f).any(axis=1))
    assert len(changed) > 0 and (ring[f[changed]] >= 0).any(axis=1).all()
    same_flip(v, f, engine, pinned=mask, band=([700], 5), crease_deg=60.0, quality_keep=0.25)


def test_shuffled_faces_change_the_result_and_still_equal_the_checker(engine):
    v, f = refined_tube()
    r = np.random.default_rng(5)
    g = f[r.permutation(len(f))]
    g = np.stack([np.roll(t, int(k)) for t, k in zip(g, r.integers(0, 3, len(g)))])
    other, rep = same_flip(v, g, engine)
    key = lambda a: sorted(tuple(sorted(t)) for t in a.tolist())          # noqa: E731
    assert rep["n_flips"] > 300 and key(other) != key(flipped("refined_tube")[2])


@settings(max_examples=40 * int(os.environ.get("MM_HYP_SCALE", "1")), deadline=None, derandomize=True, database=None,
          suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(seed=st.integers(0, 2**31 - 1), nv=st.integers(1, 12), nf=st.integers(0, 24), passes=st.integers(0, 4),
       pin=st.sampled_from([None, 0.2]), crease=st.sampled_from([30.0, 90.0]), keep=st.sampled_from([0.0, 0.5]))
def test_random_small_meshes(engine, seed, nv, nf, passes, pin, crease, keep):
    r = np.random.default_rng(seed)
    v = r.uniform(-3, 3, (nv, 3))
    f = r.integers(0, nv, (nf, 3))
    pinned = None if pin is None else r.random(nv) < pin
    same_flip(v, f, engine, passes=passes, pinned=pinned, crease_deg=crease, quality_keep=keep)
    deg, border, info = mm.mesh_valence((v, f), engine=engine)
    wdeg, wborder, winfo = FE.valence(f, nv)
    assert np.array_equal(deg, wdeg) and np.array_equal(border, wborder)
    assert all(info[k] == winfo[k] for k in ("n_edges", "n_open_edges", "n_nonmanifold_edges", "n_inconsistent_edges", "deviation"))


@pytest.mark.parametrize("name", ["refined_tube", "refined_open_tube", "messy", "jittered_tube"])
def test_mesh_valence(engine, name):
    v, f = flipped(name)[:2]
    deg, border, info = mm.mesh_valence((v, f), engine=engine)
    wdeg, wborder, winfo = FE.valence(f, len(v))
    assert deg.dtype == np.int32 and border.dtype == np.bool_ and np.array_equal(deg, wdeg) and np.array_equal(border, wborder)
    assert info == dict(n_edges=winfo["n_edges"], n_open_edges=winfo["n_open_edges"],
                        n_nonmanifold_edges=winfo["n_nonmanifold_edges"], n_inconsistent_edges=winfo["n_inconsistent_edges"],
                        deviation=winfo["deviation"], n_launches=3)
    # a face reversed: its three edges are traversed twice in one direction
    g = f.copy()
    g[0] = g[0, ::-1]
    n = mm.mesh_valence((v, g), engine=engine)[2]["n_inconsistent_edges"]
    assert n == FE.valence(g, len(v))[2]["n_inconsistent_edges"] and (n > 0 or name == "messy")     # messy: face 0's edges
    # have one or three owners


def test_face_index_out_of_range_null_engine_and_bad_numbers(engine):
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0]])
    bad = np.array([[0, 1, 2], [0, 2, 4]], dtype=np.int64)
    good = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int64)

    def raw(handle, f, crease_cos=0.5, keep=0.5, passes=3):
        out = np.full((2, 3), -77, dtype=np.int64)
        rep = N.MMFlipReport()
        C.memset(C.byref(rep), 0x5A, C.sizeof(rep))
        rc = N.lib().mm_mesh_flip_edges(handle, N._ptr(v), 4, N._ptr(f), 2, None, crease_cos, keep, passes, N._ptr(out),
                                        C.byref(rep))
        return rc, (out == -77).all() and (np.frombuffer(rep, dtype=np.uint8) == 0x5A).all()

    for handle, err in ((engine.handle, "mm_mesh_flip_edges: face index out of range"), (None, "engine == NULL")):
        rc, untouched = raw(handle, bad)
        assert rc == MM_ERR_INVALID and N.last_error() == err and untouched
    for kw in (dict(crease_cos=-0.1), dict(crease_cos=1.1), dict(crease_cos=float("nan")), dict(keep=-0.1), dict(keep=1.1),
               dict(keep=float("nan")), dict(keep=float("inf")), dict(passes=-1)):
        rc, untouched = raw(engine.handle, good, **kw)
        assert rc == MM_ERR_INVALID and untouched, kw
    assert raw(engine.handle, good)[0] == 0
    deg, border, info = np.full(4, -77, dtype=np.int32), np.full(4, 77, dtype=np.uint8), np.full(6, -77, dtype=np.int64)
    for handle, err in ((engine.handle, "mm_mesh_valence: face index out of range"), (None, "engine == NULL")):
        rc = N.lib().mm_mesh_valence(handle, None, 4, N._ptr(bad), 2, N._ptr(deg), N._ptr(border), N._ptr(info))
        assert rc == MM_ERR_INVALID and N.last_error() == err
        assert (deg == -77).all() and (border == 77).all() and (info == -77).all()


# ---- the line label -> remove -> stitch -----------------------------------------------------------------------------------

def test_stitch_with_and_without_flips(engine):
    res, geom, frames = takeoff_case(engine)
    kw = dict(region_remove="section_points", engine=engine, fill_holes=True, refine=True)
    base = mm.stitch(dict(res), geom, **kw)                               # refined: what the flips see
    again = mm.stitch(dict(res), geom, flip=False, **kw)
    assert "flip_report" not in base and sorted(base) == sorted(again)
    assert same_bits(base["mesh"][0], again["mesh"][0]) and np.array_equal(base["mesh"][1], again["mesh"][1])

    v, f = base["mesh"]
    iv = ccta._match(v, base["anomalous_points"])
    iv = np.unique(iv[iv >= 0])
    assert len(iv) > 0
    want, wrep = mm.flip_edges(base["mesh"], pinned=iv, engine=engine)
    assert wrep["n_flips"] > 0 and wrep["converged"] == 1 and wrep["n_masked_edges"] > 0
    full = mm.stitch(dict(res), geom, flip=True, relax=True, **kw)
    assert full["flip_report"] == wrep and "relax_report" in full and "refine_report" in full
    assert np.array_equal(full["mesh"][1], want[1])
    _, n_open, n_nonmanifold = SM.face_adjacency(full["mesh"][1])
    assert n_open == 0 and n_nonmanifold == 0                             # still watertight
    lumen = np.isin(f, iv).all(axis=1)
    assert lumen.sum() > 0 and np.array_equal(full["mesh"][1][lumen], f[lumen])          # the IV lumen's faces as they were
    relaxed, _, _ = mm.relax_mesh(want, engine=engine)                    # the relaxation ran behind the flips
    assert same_bits(full["mesh"][0], relaxed[0])

    two = mm.stitch_conditioned(dict(res), geom, region_remove="section_points", engine=engine, fill_holes=True, refine=True,
                                flip={"passes": 2})
    assert 1 <= two["flip_report"]["passes_run"] <= 2 and two["flip_report"]["n_flips"] > 0
    assert same_bits(two["mesh"][0], mm.stitch_conditioned(dict(res), geom, region_remove="section_points", engine=engine,
                                                           fill_holes=True, refine=True)["mesh"][0])       # no vertex moved
