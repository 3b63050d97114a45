"""Centerline from a mesh on the device (csrc/mm_geodesic_kernels.hip, csrc/mm_geodesic.cpp) against the checker
(tests/mm_checkers/mesh_skeleton.py): dist, pred, vertex_node, the node records, the node edges and the report's counts
bit for bit, at the default band and at a narrow and a wide one; the capacity retry; the composite against the
composition of the public calls and against the checker; the curved tube's centerline through prepare_centerline into
the bounded-point selection.  The fixpoint is unique, so the
tests are free of the schedule: rounds, batches and launches are only required to be plausible.  Shapes: tubes seeded by
a rim and by one vertex, two components, repeated and complete seeds, an isolated vertex, one vertex without a face, a
face with a repeated index, a grid full of ties, a NaN vertex, tubes around a workgroup (256) and a scan tile (4096), a
strip 700 hops long in index order and with its indices permuted (far more rounds than one batch, no block locality), a
large mesh followed by a small one on one engine, the refused arguments, and random soups."""
import ctypes as C

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings, strategies as st

from mm_checkers import mesh_skeleton as SK
from test_refine_host import same_bits
from test_skeleton_host import FIELD_CASES, curved_tube, field_case, trousers
from test_trim_host import octahedron

import multimoda_rs_amd as mm
from multimoda_rs_amd import _native as N

pytestmark = pytest.mark.gpu

MM_ERR_INVALID, MM_ERR_TOO_LARGE = -2, -3


def bits_equal(a, b):
    return np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


def same_field(v, f, seeds, want, engine):
    dist, pred, rep = mm.mesh_geodesic_distance((v, f), seeds, engine=engine)
    wdist, wpred, wrep = want
    assert dist.dtype == np.float64 and pred.dtype == np.int64
    assert same_bits(dist, wdist)
    assert np.array_equal(pred, wpred)
    for k in SK.GEODESIC_COUNTS:
        if isinstance(wrep[k], float):
            assert bits_equal(rep[k], wrep[k]), (k, rep[k], wrep[k])
        else:
            assert rep[k] == wrep[k], (k, rep[k], wrep[k])
    assert 1 <= rep["rounds"] <= v.shape[0] + 1 and rep["n_batches"] >= 1 and rep["n_launches"] > rep["rounds"]
    assert rep["bytes_uploaded"] == 24 * v.shape[0] + 12 * f.shape[0] + 4 * len(seeds)
    return rep


@pytest.mark.parametrize("name", sorted(FIELD_CASES))
def test_field_equals_the_checker(engine, name):
    v, f, seeds, dist, pred, report = field_case(name)
    rep = same_field(v, f, seeds, (dist, pred, report), engine)
    if name == "strip_permuted":
        assert rep["n_batches"] > 3                                      # far more rounds than one read-back
    if name == "strip":
        assert rep["rounds"] < 100                                       # about one per block of 256, not one per hop


def test_a_seed_point(engine):
    v, f, _, _, _, _ = field_case("open_tube_vertex")
    p = v[37] + [0.01, 0.0, -0.01]
    dist, pred, _ = mm.mesh_geodesic_distance((v, f), p, engine=engine)
    wdist, wpred, _ = SK.geodesic(v, f, [37])
    assert same_bits(dist, wdist) and np.array_equal(pred, wpred)


def test_a_small_mesh_after_a_large_one(engine):
    """the small call finds the large one's field, flags and adjacency at its offsets."""
    big = field_case("tube_nv_4097")
    same_field(big[0], big[1], big[2], big[3:], engine)
    for name in ("two_components", "isolated_seed", "one_vertex", "open_tube_vertex"):
        c = field_case(name)
        same_field(c[0], c[1], c[2], c[3:], engine)


def _raw(engine_handle, v, f, seeds):
    v, f, s = np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(f, dtype=np.int64), np.asarray(seeds, dtype=np.int64)
    dist, pred = np.full(max(len(v), 1), 7.0), np.full(max(len(v), 1), 7, dtype=np.int64)
    rep = N.MMGeodesicReport()
    rep.n_launches = 99
    rc = N.lib().mm_mesh_geodesic(engine_handle, N._ptr(v), len(v), N._ptr(f), len(f), N._ptr(s) if len(s) else None, len(s),
                                  N._ptr(dist), N._ptr(pred), C.byref(rep))
    return rc, N.last_error(), dist, pred, rep


@pytest.mark.parametrize("what,error", [
    ("face", "mm_mesh_geodesic: face index out of range"), ("seed_high", "mm_mesh_geodesic: seed out of range"),
    ("seed_negative", "mm_mesh_geodesic: seed out of range"), ("no_seeds", "mm_mesh_geodesic: bad arguments")])
def test_invalid_arguments_launch_nothing(engine, what, error):
    v, f = octahedron()
    seeds = [0]
    if what == "face":
        f = f.copy()
        f[3, 1] = 6
    elif what == "seed_high":
        seeds = [0, 6]
    elif what == "seed_negative":
        seeds = [-1]
    else:
        seeds = []
    rc, err, dist, pred, rep = _raw(engine.handle, v, f, seeds)
    assert rc == MM_ERR_INVALID and err == error
    assert (dist == 7.0).all() and (pred == 7).all() and rep.n_launches == 99          # nothing written


def test_null_engine_and_no_vertices(engine):
    v, f = octahedron()
    rc, err, _, _, _ = _raw(None, v, f, [0])
    assert rc == MM_ERR_INVALID and err == "engine == NULL"
    rc, err, _, _, _ = _raw(engine.handle, np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64), [0])
    assert rc == MM_ERR_INVALID and err == "mm_mesh_geodesic: seed out of range"


@st.composite
def soups(draw):
    nv = draw(st.integers(1, 40))
    nf = draw(st.integers(0, 80))
    coord = st.sampled_from([0.0, 1.0, 2.0, 0.5, -1.5, 3.25, 1e-3, 7.0])   # few values: repeated points, zero edges
    v = np.array(draw(st.lists(st.tuples(coord, coord, coord), min_size=nv, max_size=nv)), dtype=np.float64).reshape(nv, 3)
    idx = st.integers(0, nv - 1)
    f = np.array(draw(st.lists(st.tuples(idx, idx, idx), min_size=nf, max_size=nf)), dtype=np.int64).reshape(nf, 3)
    seeds = draw(st.lists(idx, min_size=1, max_size=5))
    return v, f, seeds


@settings(max_examples=40, deadline=None, derandomize=True, database=None, suppress_health_check=list(HealthCheck))
@given(soups())
def test_soups(engine, soup):
    v, f, seeds = soup
    same_field(v, f, np.array(seeds, dtype=np.int64), SK.geodesic(v, f, seeds), engine)


# ---- Rule S ----------------------------------------------------------------------------------------------------------------

NODE_FLOATS = ("x", "y", "z", "radius", "radius_min", "weight")
NODE_INTS = ("band", "first_vertex", "n_vertices", "flags")


def same_skeleton(v, f, seeds, band, engine):
    got = mm.mesh_skeleton((v, f), seeds, band_mm=band, engine=engine)
    want = SK.skeleton(v, f, seeds, SK.default_band(v, f) if band is None else band)
    assert same_bits(got.dist, want["dist"]) and np.array_equal(got.pred, want["pred"])
    assert got.vertex_node.dtype == np.int64 and np.array_equal(got.vertex_node, want["vertex_node"])
    assert got.nodes.dtype == SK.NODE_DTYPE and len(got.nodes) == len(want["nodes"])
    for k in NODE_FLOATS:
        assert same_bits(got.nodes[k], want["nodes"][k]), k
    for k in NODE_INTS:
        assert np.array_equal(got.nodes[k], want["nodes"][k]), k
    assert got.edges.dtype == np.int64 and np.array_equal(got.edges, want["edges"])
    rep = got.report
    assert rep["n_nodes"] == want["report"]["n_nodes"] and rep["n_node_edges"] == want["report"]["n_node_edges"]
    for k in SK.GEODESIC_COUNTS:
        assert bits_equal(rep["field"][k], want["report"][k]) if isinstance(want["report"][k], float) else \
            rep["field"][k] == want["report"][k], k
    assert rep["n_launches"] > rep["field"]["rounds"] and rep["union_rounds"] >= 1
    return got, want


SKELETON_CASES = [n for n in sorted(FIELD_CASES) if n not in ("one_vertex", "nan_vertex", "strip", "strip_permuted")]


@pytest.mark.parametrize("name", SKELETON_CASES)
def test_skeleton_equals_the_checker(engine, name):
    v, f, seeds = field_case(name)[:3]
    same_skeleton(v, f, seeds, None, engine)


@pytest.mark.parametrize("name,scale", [("wound_tube_vertex", 0.3), ("wound_tube_vertex", 3.0), ("open_tube_rim", 0.25),
                                        ("trousers", 0.4), ("grid", 0.5), ("grid", 1.0), ("tube_nv_4097", 0.2),
                                        ("repeated_index", 0.7), ("two_components", 5.0)])
def test_skeleton_at_other_bands(engine, name, scale):
    v, f, seeds = field_case(name)[:3]
    got, want = same_skeleton(v, f, seeds, scale * SK.default_band(v, f), engine)
    if name == "tube_nv_4097":
        assert len(got.nodes) > 256                                         # more nodes than one workgroup and one sort tile


def test_skeleton_special_cases(engine):
    v, f, seeds = field_case("one_vertex")[:3]
    got, _ = same_skeleton(v, f, seeds, 1.0, engine)                      # nv = 1, nf = 0: one node by the plain mean
    assert len(got.nodes) == 1 and got.nodes["flags"][0] == 2 | 4 and len(got.edges) == 0
    v, f, seeds = field_case("nan_vertex")[:3]
    got, _ = same_skeleton(v, f, seeds, None, engine)                     # the NaN's faces make their nodes take the plain mean
    assert (got.nodes["flags"] & 2).any() and got.vertex_node[3] == -1 and np.isfinite(got.nodes["x"]).all()
    v, f, seeds = field_case("strip_permuted")[:3]
    same_skeleton(v, f, seeds, 25.0, engine)


def test_a_small_skeleton_after_a_large_one(engine):
    v, f, seeds = field_case("tube_nv_4097")[:3]
    same_skeleton(v, f, seeds, 0.3 * SK.default_band(v, f), engine)
    for name in ("two_components", "isolated_seed", "open_tube_vertex"):
        v, f, seeds = field_case(name)[:3]
        same_skeleton(v, f, seeds, None, engine)


def _raw_skeleton(handle, v, f, seeds, band, node_cap, edge_cap):
    v, f, s = np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(f, dtype=np.int64), np.asarray(seeds, dtype=np.int64)
    nv = len(v)
    out = {"dist": np.full(nv, 7.0), "pred": np.full(nv, 7, dtype=np.int64), "vertex_node": np.full(nv, 7, dtype=np.int64),
           "nodes": np.zeros(max(node_cap, 1), dtype=SK.NODE_DTYPE), "edges": np.full((max(edge_cap, 1), 2), 7, dtype=np.int64)}
    rep = N.MMSkeletonReport()
    rep.n_launches = 99
    rc = N.lib().mm_mesh_skeleton(handle, N._ptr(v), nv, N._ptr(f), len(f), N._ptr(s) if len(s) else None, len(s), band, node_cap,
                                  edge_cap, N._ptr(out["dist"]), N._ptr(out["pred"]), N._ptr(out["vertex_node"]),
                                  N._ptr(out["nodes"]), N._ptr(out["edges"]), C.byref(rep))
    return rc, N.last_error(), out, rep


def _untouched(out, rep):
    return (out["dist"] == 7.0).all() and (out["pred"] == 7).all() and (out["vertex_node"] == 7).all() and \
        (out["edges"] == 7).all() and not out["nodes"]["n_vertices"].any() and rep.n_launches == 99


def test_capacity_retry(engine):
    v, f, seeds = field_case("wound_tube_vertex")[:3]
    band = SK.default_band(v, f)
    want = SK.skeleton(v, f, seeds, band)
    k, m = len(want["nodes"]), len(want["edges"])
    for node_cap, edge_cap in ((k - 1, m), (k, m - 1), (0, 0)):
        rc, err, out, rep = _raw_skeleton(engine.handle, v, f, seeds, band, node_cap, edge_cap)
        assert rc == MM_ERR_TOO_LARGE and "too small" in err and rep.n_nodes == k and rep.n_node_edges == m
        assert (out["dist"] == 7.0).all() and (out["vertex_node"] == 7).all() and (out["edges"] == 7).all()
    rc, err, out, rep = _raw_skeleton(engine.handle, v, f, seeds, band, k, m)
    assert rc == 0 and np.array_equal(out["edges"], want["edges"]) and np.array_equal(out["vertex_node"], want["vertex_node"])
    assert same_bits(out["nodes"]["x"], want["nodes"]["x"])


@pytest.mark.parametrize("what", ["band_zero", "band_negative", "band_nan", "band_inf", "seed", "no_seeds", "face"])
def test_invalid_skeleton_arguments_launch_nothing(engine, what):
    v, f = octahedron()
    f = f.copy()
    seeds, band = [0], 1.0
    if what.startswith("band"):
        band = {"band_zero": 0.0, "band_negative": -1.0, "band_nan": float("nan"), "band_inf": float("inf")}[what]
    elif what == "seed":
        seeds = [6]
    elif what == "no_seeds":
        seeds = []
    else:
        f[0, 0] = -1
    rc, err, out, rep = _raw_skeleton(engine.handle, v, f, seeds, band, 16, 16)
    assert rc == MM_ERR_INVALID and err.startswith("mm_mesh_skeleton: ")
    assert _untouched(out, rep)


def test_a_band_index_past_the_int32_range(engine):
    v, f = octahedron()
    rc, err, out, rep = _raw_skeleton(engine.handle, v, f, [0], 1e-10, 16, 16)
    assert rc == MM_ERR_TOO_LARGE and err == "mm_mesh_skeleton: a band index passes 2^31"
    assert (out["vertex_node"] == 7).all() and (out["dist"] == 7.0).all()
    with pytest.raises(OverflowError):
        SK.skeleton(v, f, [0], 1e-10)


@settings(max_examples=40, deadline=None, derandomize=True, database=None, suppress_health_check=list(HealthCheck))
@given(soups(), st.sampled_from([0.3, 1.0, 2.5, 40.0]))
def test_skeleton_soups(engine, soup, band):
    v, f, seeds = soup
    same_skeleton(v, f, np.array(seeds, dtype=np.int64), band, engine)


# ---- the composite ---------------------------------------------------------------------------------------------------------

def same_centerline(a, b):
    assert len(a) == len(b)
    for k in ("x", "y", "z", "tx", "ty", "tz", "radius"):
        assert same_bits(a.points[k], b.points[k]), k
    assert np.array_equal(a.points["branch_id"], b.points["branch_id"])


COMPOSITE = {"trousers": lambda: (trousers(noise=0.05, seed=2)[:2], trousers()[2]["seeds"]),
             "curved_tube": lambda: (curved_tube(2)[:2], curved_tube(2)[2]),
             "open_tube_vertex": lambda: (field_case("open_tube_vertex")[:2], [254]),
             "wound_tube_vertex": lambda: (field_case("wound_tube_vertex")[:2], [100])}


@pytest.mark.parametrize("name", sorted(COMPOSITE))
def test_centerline_from_mesh_is_the_composition_of_the_public_calls(engine, name):
    (v, f), seeds = COMPOSITE[name]()
    cl, rep = mm.centerline_from_mesh((v, f), seeds, engine=engine)
    graph = mm.mesh_skeleton((v, f), seeds, engine=engine)
    rings = mm.order_boundary_rings(f, v, engine=engine)
    terminals = mm.skeleton.skeleton_terminals(v, rings, seeds, graph.vertex_node)
    want, wrep = mm.skeleton_centerline(graph.nodes, graph.edges, terminals)
    same_centerline(cl, want)
    assert rep["branches"] == wrep["branches"] and np.array_equal(rep["point_node"], wrep["point_node"])
    assert np.array_equal(rep["graph"].vertex_node, graph.vertex_node) and len(rep["terminals"]) == len(terminals)
    # and the checker's composite, which finds the rims on its own
    check = SK.centerline(v, f, seeds)
    for c, k in enumerate(("x", "y", "z", "radius")):
        assert same_bits(cl.points[k], [p[c] for p in check["points"]]), k
    assert cl.points["branch_id"].tolist() == [p[4] for p in check["points"]]
    assert [(b["parent_branch"], b["parent_index"], int(b["ends_at_rim"]), b["n_points"]) for b in rep["branches"]] == check["branches"]
    for k, x in check["report"].items():
        assert rep[k] == x, k
    # the optional steps are the existing methods, in order
    again, _ = mm.centerline_from_mesh((v, f), seeds, spacing_mm=0.7, smooth_sigma=1.5, engine=engine)
    same_centerline(again, cl.resample(0.7).smooth(1.5))


def test_trousers_on_the_device(engine):
    v, f, info = trousers(noise=0.05, seed=3)
    cl, rep = mm.centerline_from_mesh((v, f), info["seeds"], engine=engine)
    assert rep["n_terminals"] == 2 and rep["n_loops"] == 0 and rep["n_branches"] == 2
    assert rep["branches"][1]["parent_branch"] == 0 and all(b["ends_at_rim"] for b in rep["branches"])
    starts = cl.branch_start_indices
    assert starts == [0, rep["branches"][0]["n_points"]] and 0 <= rep["branches"][1]["parent_index"] < starts[1]


def test_the_curved_tube_feeds_the_labelling(engine, capsys):
    v, f, seeds = curved_tube(1)
    cl, rep = mm.centerline_from_mesh((v, f), seeds, engine=engine)
    assert rep["n_branches"] == 1
    ready = mm.prepare_centerline(mm.load_centerline(cl.get_branch(0), "curved tube"))
    inside = mm.find_centerline_bounded_points_simple(ready, v, 1.5 * 2.0, engine=engine)
    assert len(inside) == len(v)
