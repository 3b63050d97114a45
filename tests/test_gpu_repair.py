"""The mesh repair on the device (csrc/mm_repair_kernels.hip, csrc/mm_repair.cpp) against its checker
(tests/mm_checkers/repair_mesh.py): vertex bits, faces, origin, target and every count of the report on the shapes of
tests/test_repair_host.py, each switch off on its own, the capacity retry through the C ABI, stale scratch, random face
soups, and the line: mm.stitch(repair=True) and mm.fix_and_remesh_stitched_mesh as compositions of the public calls.
union_rounds, n_launches and the byte counts are not in the checker: they are held against the header's formulas."""
import ctypes as C
import os

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings, strategies as st

from mm_checkers import repair_mesh as RM
from test_refine_host import same_bits, wound_tube
from test_repair_host import (SHAPES, CLEAN, cones, duplicates, five_on_an_edge, kept_by_one_edge_removed_by_another,
                              pinched_rim, solids_at_a_vertex, solids_at_an_edge, soup)
from test_gpu_stitch import takeoff_case

import multimoda_rs_amd as mm
from multimoda_rs_amd import ccta

pytestmark = pytest.mark.gpu

N = mm._native
MM_ERR_INVALID, MM_ERR_TOO_LARGE = -2, -3


def same_repair(v, f, engine, **kw):
    """mm.repair_mesh equals the checker; returns the device's result."""
    v, f = np.asarray(v, dtype=np.float64).reshape(-1, 3), np.asarray(f, dtype=np.int64).reshape(-1, 3)
    wv, wf, worigin, wtarget, wrep = RM.repair(v, f, **kw)
    v0, f0 = v.copy(), f.copy()
    (gv, gf), origin, target, rep = mm.repair_mesh((v, f), engine=engine, **kw)
    assert same_bits(v, v0) and np.array_equal(f, f0)                      # the input is untouched
    assert same_bits(gv, wv) and np.array_equal(gf, wf) and gf.dtype == np.int64
    assert np.array_equal(origin, worigin) and np.array_equal(target, wtarget)
    assert {k: rep[k] for k in RM.COUNT_KEYS} == wrep
    assert rep["watertight"] == (wrep["n_open_edges_after"] == 0 and wrep["n_nonmanifold_edges_after"] == 0)
    assert 0 <= rep["union_rounds"] <= RM.rounds_bound(len(f))
    if len(v) == 0:
        assert rep["n_launches"] == 0 and rep["bytes_uploaded"] == 0
    else:
        assert rep["n_launches"] == (RM.LAUNCHES if len(f) else RM.LAUNCHES - 6) + rep["union_rounds"]
        assert rep["bytes_uploaded"] == 24 * len(v) + 12 * len(f)
        assert rep["bytes_downloaded"] == 28 * len(gv) + 12 * len(gf) + 4 * len(v) + 152
    return (gv, gf), origin, target, rep


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_equal_the_checker(engine, name):
    same_repair(*SHAPES[name](), engine)


@pytest.mark.parametrize("name", sorted(CLEAN))
def test_clean_meshes_come_back_bit_for_bit(engine, name):
    v, f = CLEAN[name]()
    (gv, gf), origin, target, rep = same_repair(v, f, engine)
    assert same_bits(gv, v) and np.array_equal(gf, f) and np.array_equal(origin, np.arange(len(v)))
    assert np.array_equal(target, origin) and rep["n_faces_removed"] == rep["n_new_vertices"] == rep["n_welded_vertices"] == 0


def test_five_on_an_edge_keeps_the_two_largest(engine):
    (_, gf), _, _, rep = same_repair(*five_on_an_edge(), engine)
    assert gf.tolist() == [[1, 0, 5], [0, 1, 6]] and rep["n_faces_removed"] == 3
    (_, gf), _, _, _ = same_repair(*five_on_an_edge((3.0, 3.0, 3.0, 1.0, 1.0)), engine)
    assert gf.tolist() == [[1, 0, 3], [0, 1, 4]]                          # the index breaks the tie
    (_, shuffled), _, _, _ = same_repair(*five_on_an_edge(order=(3, 0, 4, 2, 1)), engine)
    assert {tuple(r) for r in shuffled.tolist()} == {(1, 0, 5), (0, 1, 6)}


def test_a_face_kept_by_one_edge_and_removed_by_another_leaves_an_open_edge(engine):
    (_, gf), _, _, rep = same_repair(*kept_by_one_edge_removed_by_another(), engine)
    assert rep["n_faces_removed"] == 2 and len(gf) == 3
    assert rep["n_open_edges_after"] == 7 and rep["n_open_edges_before"] == 9       # 1 - 2 is left with one owner


def test_vertex_splits(engine):
    (gv, gf), origin, _, rep = same_repair(*solids_at_a_vertex(), engine)
    assert rep["n_nonmanifold_vertices"] == 1 and rep["n_new_vertices"] == 1 and origin[-1] == 0 and same_bits(gv[-1], gv[0])
    (gv, gf), origin, _, rep = same_repair(*solids_at_a_vertex(3, shuffle=5), engine)
    assert rep["n_nonmanifold_vertices"] == 1 and rep["n_new_vertices"] == 2 and origin[-2:].tolist() == [0, 0]
    firsts = [min(i for i, row in enumerate(gf.tolist()) if x in row) for x in (0, 10, 11)]
    assert firsts == sorted(firsts)                                       # numbered by the smallest corner
    _, _, _, rep = same_repair(*solids_at_an_edge(), engine)                # (d) and (e) together
    assert rep["n_faces_removed"] == 2 and rep["n_new_vertices"] == 2 and rep["n_open_edges_after"] == 4


def test_the_pinched_rim_closes_after_the_repair(engine):
    v, f = pinched_rim()
    before = mm.fill_holes(v, f, engine=engine)[2]
    assert before["n_irregular_components"] > 0 and not before["watertight"]
    assert mm.mesh_manifold_report((v, f), engine)["n_nonmanifold_vertices"] == 1
    (gv, gf), _, _, rep = same_repair(v, f, engine)
    assert rep["n_new_vertices"] == 1
    after = mm.fill_holes(gv, gf, engine=engine)[2]
    assert after["n_irregular_components"] == 0 and after["n_loops_filled"] == 2 and after["watertight"]


def test_a_repaired_mesh_needs_nothing(engine):
    for name in ("two_solids_at_a_vertex", "three_solids_out_of_order", "two_solids_at_an_edge", "pinched_rim", "soup"):
        first = mm.repair_mesh(SHAPES[name](), engine=engine)[0]
        for kw in ({}, {"nonmanifold_vertices": False}):
            (gv, gf), origin, target, rep = same_repair(first[0], first[1], engine, **kw)
            assert same_bits(gv, first[0]) and np.array_equal(gf, first[1]), name
            assert np.array_equal(origin, np.arange(len(gv))) and np.array_equal(target, origin)
            assert rep["n_welded_vertices"] == rep["n_new_vertices"] == rep["n_nonmanifold_vertices"] == 0
    v, f = first = mm.repair_mesh(solids_at_a_vertex(), engine=engine)[0]
    g = f.copy()
    g[0][g[0] == 0] = 7                                                    # the copy named by a face of the other solid
    _, _, target, rep = same_repair(v, g, engine)
    assert rep["n_welded_vertices"] == 1 and target[7] == 0 and rep["n_new_vertices"] == 1


def test_duplicates(engine):
    v, f = duplicates()
    (gv, _), origin, target, rep = same_repair(v, f, engine)
    assert rep["n_welded_vertices"] == 3 and target[[6, 7, 9]].tolist() == [2, 0, 4] and target[8] == 6
    assert rep["n_degenerate_faces"] == 2 and rep["n_null_faces"] == 1 and rep["n_duplicate_faces"] == 6
    assert gv[0].view(np.uint64).tolist() == [0, 0, 0]                    # the survivor's bits, not the -0.0's
    _, _, target, rep = same_repair(v, f, engine, drop_unreferenced=True)
    assert rep["n_unreferenced_dropped"] == 2 and target[5] == -1 and target[10] == -1


@pytest.mark.parametrize("off", RM.FLAGS)
@pytest.mark.parametrize("name", ["duplicates", "two_solids_at_an_edge", "soup"])
def test_each_switch_on_its_own(engine, name, off):
    kw = {off: off == "drop_unreferenced"}                                 # the one switch that is off by default: on
    same_repair(*SHAPES[name](), engine, **kw)


def test_manifold_report_counts_and_changes_nothing(engine):
    for name in ("duplicates", "two_solids_at_an_edge", "pinched_rim", "soup"):
        v, f = SHAPES[name]()
        got = mm.mesh_manifold_report((v, f), engine)
        want = RM.manifold_counts(v, f)
        assert {k: got[k] for k in ccta.MANIFOLD_REPORT_KEYS} == want, name
        assert got["watertight"] == (want["n_open_edges"] == 0 and want["n_nonmanifold_edges"] == 0)
    assert mm.mesh_manifold_report(wound_tube(15, 17), engine)["watertight"]


def test_two_cones_at_one_apex(engine):
    """30000 corners: past one scan tile and many workgroups; the shuffled cone makes the union-find's trees deep."""
    v, f = cones()
    (gv, gf), origin, _, rep = same_repair(v, f, engine)
    assert rep["n_new_vertices"] == 1 and rep["n_nonmanifold_vertices"] == 1 and origin[-1] == 0
    assert rep["union_rounds"] >= 1 and rep["union_rounds"] <= RM.rounds_bound(len(f))
    assert rep["n_launches"] == RM.LAUNCHES + rep["union_rounds"]
    assert (gf[:5000] != len(v)).all() and (gf[5000:, 0] == len(v)).all()


def test_other_sizes(engine):
    same_repair(*cones(257, second=False), engine)                         # one face past a workgroup
    v = cones(257, second=False)[0]
    (gv, gf), origin, target, rep = same_repair(np.concatenate([v[:5], v[:2]]), np.zeros((0, 3), dtype=np.int64), engine)
    assert len(gv) == 5 and len(gf) == 0 and target.tolist() == [0, 1, 2, 3, 4, 0, 1] and rep["union_rounds"] == 0
    (gv, gf), origin, target, rep = same_repair(np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64), engine)
    assert len(gv) == len(gf) == len(origin) == len(target) == 0


def raw_repair(handle, v, f, flags, vert_cap):
    nv, nf = len(v), len(f)
    ov, of = np.full((max(vert_cap, 1), 3), -77.0), np.full((max(nf, 1), 3), -77, dtype=np.int64)
    origin, target = np.full(max(vert_cap, 1), -77, dtype=np.int64), np.full(max(nv, 1), -77, dtype=np.int64)
    rep = N.MMRepairReport()
    C.memset(C.byref(rep), 0x5A, C.sizeof(rep))
    rc = N.lib().mm_mesh_repair(handle, N._ptr(v), nv, N._ptr(f), nf, flags, vert_cap, N._ptr(ov), N._ptr(of),
                                N._ptr(origin), N._ptr(target), C.byref(rep))
    untouched = (ov == -77).all() and (of == -77).all() and (origin == -77).all() and (target == -77).all()
    return rc, rep, untouched, (ov, of, origin, target)


def test_the_capacity_retry_and_the_rejections(engine):
    v, f = solids_at_a_vertex()
    v, f = np.ascontiguousarray(v), np.ascontiguousarray(f, dtype=np.int64)
    rc, rep, untouched, _ = raw_repair(engine.handle, v, f, 31, len(v))
    assert rc == MM_ERR_TOO_LARGE and untouched and rep.n_vertices == len(v) + 1 and rep.n_faces == len(f)
    assert rep.n_new_vertices == 1
    rc, rep2, _, (ov, of, origin, target) = raw_repair(engine.handle, v, f, 31, int(rep.n_vertices))
    want = RM.repair(v, f)
    assert rc == 0 and same_bits(ov, want[0]) and np.array_equal(of, want[1]) and np.array_equal(origin, want[2])

    def report_untouched(r):
        return (np.frombuffer(r, dtype=np.uint8) == 0x5A).all()

    bad_f = f.copy()
    bad_f[3, 1] = len(v)
    bad_v = v.copy()
    bad_v[2, 1] = np.inf
    for args, err in (((engine.handle, v, bad_f, 31, 16), "mm_mesh_repair: face index out of range"),
                      ((engine.handle, bad_v, f, 31, 16), "mm_mesh_repair: non-finite coordinate"),
                      ((engine.handle, v, f, 64, 16), "mm_mesh_repair: bad arguments"),
                      ((None, v, f, 31, 16), "engine == NULL")):
        rc, rep, untouched, _ = raw_repair(*args)
        assert rc == MM_ERR_INVALID and N.last_error() == err and untouched and report_untouched(rep)


def test_stale_scratch_never_reaches_a_result(engine):
    big = cones()
    small = solids_at_a_vertex()
    fresh = mm.Engine()
    try:
        want = mm.repair_mesh(small, engine=fresh)
    finally:
        fresh.close()
    mm.repair_mesh(big, engine=engine)
    for _ in range(2):                                                     # behind the large mesh, and the same call again
        got = mm.repair_mesh(small, engine=engine)
        assert same_bits(got[0][0], want[0][0]) and np.array_equal(got[0][1], want[0][1])
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        assert {k: got[3][k] for k in RM.COUNT_KEYS} == {k: want[3][k] for k in RM.COUNT_KEYS}


@settings(max_examples=40 * int(os.environ.get("MM_HYP_SCALE", "1")), deadline=None, derandomize=True, database=None,
          suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(seed=st.integers(0, 2**31 - 1), drop=st.booleans(), off=st.sampled_from([None] + list(RM.FLAGS[:5])))
def test_random_face_soups(engine, seed, drop, off):
    kw = {"drop_unreferenced": drop}
    if off is not None:
        kw[off] = False
    same_repair(*soup(seed), engine, **kw)


# ---- the line ---------------------------------------------------------------------------------------------------------------

def test_stitch_with_and_without_repair(engine):
    res, geom, _ = takeoff_case(engine)
    kw = dict(region_remove="section_points", engine=engine)
    base = mm.stitch(dict(res), geom, fill_holes=True, **kw)
    again = mm.stitch(dict(res), geom, fill_holes=True, repair=False, **kw)
    assert "repair" not in base and sorted(base) == sorted(again)
    assert same_bits(base["mesh"][0], again["mesh"][0]) and np.array_equal(base["mesh"][1], again["mesh"][1])

    open_mesh = mm.stitch(dict(res), geom, **kw)["mesh"]                   # the three calls by hand
    repaired, _, _, r_repair = mm.repair_mesh(open_mesh, engine=engine)
    fv, ff, r_fill = mm.fill_holes(repaired[0], repaired[1], engine=engine)
    full = mm.stitch(dict(res), geom, fill_holes=True, repair=True, **kw)
    assert {k: full["repair"][k] for k in RM.COUNT_KEYS} == {k: r_repair[k] for k in RM.COUNT_KEYS}
    assert same_bits(full["mesh"][0], fv) and np.array_equal(full["mesh"][1], ff)
    assert {k: v for k, v in full["fill_report"].items() if k != "winding_rounds"} == \
        {k: v for k, v in r_fill.items() if k != "winding_rounds"}
    cond = mm.stitch_conditioned(dict(res), geom, fill_holes=True, repair={"drop_unreferenced": True}, **kw)
    assert "repair" in cond and cond["repair"]["n_nonmanifold_edges_after"] == 0


def damaged_tube():
    """wound_tube(15, 17) without its top cap, with a small fin on a wall edge and a small tetrahedron that touches the
    wall in one vertex."""
    v, f = wound_tube(15, 17)
    f = f[:-15]                                                            # the top cap's faces are the last
    a, b = int(f[40, 0]), int(f[40, 1])
    fin_apex = 0.5 * (v[a] + v[b]) * [1.1, 1.1, 1.0]
    at = v[100]
    tet = at + np.array([[0.2, 0.0, 0.0], [0.2, 0.1, 0.1], [0.25, -0.1, 0.1]]) * np.sign(at[0] if at[0] != 0 else 1.0)
    nv = len(v)
    v = np.concatenate([v, [fin_apex], tet])
    t = [100, nv + 1, nv + 2, nv + 3]
    extra = [[a, b, nv], [t[0], t[1], t[2]], [t[0], t[3], t[1]], [t[0], t[2], t[3]], [t[1], t[3], t[2]]]
    return v, np.concatenate([f, np.array(extra)])


def test_fix_and_remesh_is_the_public_calls_and_ends_watertight(engine):
    v, f = damaged_tube()
    found = mm.mesh_manifold_report((v, f), engine)
    assert found["n_nonmanifold_edges"] == 1 and found["n_open_edges"] == 15 + 2      # the cap's rim, the fin's two sides
    assert found["n_nonmanifold_vertices"] == 3                            # the bow-tie, and the fin's corners at a and b
    pinned = np.zeros(len(v), dtype=bool)
    pinned[30:45] = True                                                   # one ring of the wall
    pinned[100] = True                                                     # the vertex the split doubles
    (gv, gf), rep = mm.fix_and_remesh_stitched_mesh((v, f), remesh_iterations=2, pinned=pinned, return_report=True,
                                                    engine=engine)
    after = mm.mesh_manifold_report((gv, gf), engine)
    assert after["watertight"] and after["n_nonmanifold_edges"] == 0 and after["n_nonmanifold_vertices"] == 0
    assert rep["watertight"] and (ccta._match(gv, v[pinned]) >= 0).all()   # no pinned vertex vanished or moved

    L = mm.edge_length_target((v, f), engine=engine)
    assert rep["target_edge_length_mm"] == L
    cur, origin, _, r0 = mm.repair_mesh((v, f), engine=engine)
    mask = pinned[origin]
    assert mask.sum() == pinned.sum() + 1                                  # the new vertex inherits its parent's pin
    fv, ff, r1 = mm.fill_holes(cur[0], cur[1], engine=engine)
    mask = np.concatenate([mask, np.zeros(len(fv) - len(mask), dtype=bool)])
    cur, r2 = mm.isotropic_remesh((fv, ff), L, iterations=2, pinned=mask, engine=engine)
    loose = ("union_rounds", "n_launches", "winding_rounds")
    strip = lambda d: {k: x for k, x in d.items() if k not in loose}        # noqa: E731
    assert strip(rep["repair"]) == strip(r0) and strip(rep["fill"]) == strip(r1)
    assert len(rep["remesh"]["iterations"]) == 2 and rep["remesh"]["n_faces_after"] == r2["n_faces_after"]
    if rep["post_repair"] is None:
        assert same_bits(gv, cur[0]) and np.array_equal(gf, cur[1])
    else:
        cur, _, _, r3 = mm.repair_mesh(cur, duplicate_vertices=False, engine=engine)
        fv, ff, r4 = mm.fill_holes(cur[0], cur[1], engine=engine)
        assert same_bits(gv, fv) and np.array_equal(gf, ff) and strip(rep["post_repair"]) == strip(r3)
