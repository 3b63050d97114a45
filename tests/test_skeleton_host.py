"""Centerline from a mesh, host side (include/mm_centerline.h, rules G, S and T; tests/mm_checkers/mesh_skeleton.py): the
checker's Dijkstra against its own Jacobi sweep and scipy's Dijkstra, bit for bit; mm_skeleton_centerline (host C++)
against the checker on hand-made node graphs; the rule's geometry on a curved tube and a pair of trousers, on the
checker (a cap that keeps the rule honest, not a measurement of the device); the public names; the arguments refused
before the device is touched.  The shapes here are shared with tests/test_gpu_skeleton.py.

Worst distances from the true axis measured with this checker: curved tube 0.072, 0.089, 0.073 mm of a radius of 2.0
(noise seeds 1, 2, 3; cap 0.2); trousers' legs 0.036 mm without noise and 0.044, 0.074, 0.072, 0.056 mm of 1.3 with
noise seeds 1 .. 4 (cap 0.13)."""
import functools
import inspect

import numpy as np
import pytest

from mm_checkers import mesh_skeleton as SK
from test_trim_host import octahedron
from test_gpu_branch_label import tube
from test_refine_host import jitter, open_tube, same_bits, wound_tube

import multimoda_rs_amd as mm


# ---- shapes ------------------------------------------------------------------------------------------------------------

def strip(n=700, permute_seed=None):
    """A strip of 2 x n vertices, n - 1 quads cut in two: a path n - 1 hops long.  With a seed the vertex indices are
    randomly permuted, so no two neighbours share a block of consecutive indices.  Vertex 0 of the unpermuted strip is
    returned as the third item."""
    x = np.arange(n, dtype=np.float64)
    v = np.concatenate([np.stack([x, np.zeros(n), np.zeros(n)], 1), np.stack([x + 0.25, np.ones(n), np.zeros(n)], 1)])
    i = np.arange(n - 1)
    f = np.concatenate([np.stack([i, i + 1, n + i], 1), np.stack([i + 1, n + i + 1, n + i], 1)]).astype(np.int64)
    if permute_seed is None:
        return v, f, 0
    p = np.random.default_rng(permute_seed).permutation(2 * n)           # old index -> new index
    out = np.empty_like(v)
    out[p] = v
    return out, p[f], int(p[0])


def grid(n=12):
    """n x n unit squares cut along one diagonal: many paths of equal length to most vertices."""
    j, i = np.meshgrid(np.arange(n + 1), np.arange(n + 1))
    v = np.stack([i.ravel().astype(float), j.ravel().astype(float), np.zeros((n + 1) ** 2)], 1)
    q = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
    f = np.concatenate([np.stack([q, q + 1, q + n + 2], 1), np.stack([q, q + n + 2, q + n + 1], 1)]).astype(np.int64)
    return v, f


def two_components():
    v, f = octahedron()
    return np.concatenate([v, v * 0.5 + [10.0, 0, 0]]), np.concatenate([f, f + 6])


def with_isolated_vertex():
    v, f = octahedron()
    return np.concatenate([v, [[3.0, 3.0, 3.0]]]), f


def with_repeated_index():
    v, f = octahedron()
    return v, np.concatenate([f, [[2, 2, 5], [4, 1, 4]]])


def with_nan_vertex():
    """Vertex 3 of a jittered tube is NaN: its edges are skipped and it stays unreached."""
    v, f = wound_tube(9, 6)
    v = jitter(v, 2)
    v[3] = np.nan
    return v, f


def _strip(lower, upper):
    """the faces between two loops of equal length given as index lists"""
    n = len(lower)
    f = []
    for k in range(n):
        a, b, c, d = lower[k], lower[(k + 1) % n], upper[(k + 1) % n], upper[k]
        f += [(a, b, d), (b, c, d)]
    return f


def curved_tube(seed, n_rings=120, n_ring=28):
    """tube() of test_gpu_branch_label.py about a quarter arc of radius 20 in z = 0, tube radius 2, vertex noise 0.03:
    (vertices, faces, the first ring)."""
    t = np.linspace(0.0, np.pi / 2.0, n_rings)
    v = tube(np.stack([20.0 * np.cos(t), 20.0 * np.sin(t), np.zeros_like(t)], 1), 2.0, n_ring)
    v = v + np.random.default_rng(seed).normal(0.0, 0.03, v.shape)
    f = []
    for i in range(n_rings - 1):
        f += _strip(list(range(i * n_ring, (i + 1) * n_ring)), list(range((i + 1) * n_ring, (i + 2) * n_ring)))
    return v, np.array(f, dtype=np.int64), list(range(n_ring))


def trousers(m=12, waist_radius=2.0, leg_radius=1.3, trunk_rings=14, leg_rings=(30, 22), step=0.45, sag=0.8, splay_deg=25.0,
             noise=0.0, seed=0):
    """A manifold pair of trousers: a waist ring of 2 m vertices in z = 0, a bridge of m - 1 vertices sagging between waist
    vertices 0 and m, a trunk extruded up from the waist, and two legs whose first loop is one half of the waist plus the
    bridge, extruded along their own direction and blended to a circle over four rings; legs of different length.
    Returns (vertices, faces, info): info holds the seed ring (the trunk's top) and, per leg, (axis origin, direction, the
    distance along the axis where the blend ends)."""
    n = 2 * m
    th = 2.0 * np.pi * np.arange(n) / n
    v = [np.stack([waist_radius * np.cos(th), waist_radius * np.sin(th), np.zeros(n)], 1)]
    waist = list(range(n))
    j = np.arange(1, m)
    v.append(np.stack([waist_radius * (1.0 - 2.0 * j / m), np.zeros(m - 1), -sag * np.sin(np.pi * j / m)], 1))
    bridge = list(range(n, n + m - 1))
    count = n + m - 1
    faces = []
    prev = waist
    for r in range(1, trunk_rings + 1):
        v.append(v[0] + [0.0, 0.0, r * step])
        ring = list(range(count, count + n))
        count += n
        faces += _strip(prev, ring)
        prev = ring
    top = prev
    loops = [waist[:m + 1] + bridge[::-1], waist[m:] + [waist[0]] + bridge]
    legs = []
    base = np.concatenate(v)
    phi = np.radians(splay_deg)
    for side, (loop, rings) in enumerate(zip(loops, leg_rings)):
        d = np.array([0.0, np.sin(phi) * (1 if side == 0 else -1), -np.cos(phi)])
        u = np.array([1.0, 0.0, 0.0])
        w = np.cross(d, u)
        p0 = base[loop]
        c = p0.mean(axis=0)
        q = p0 - c
        a0, a1 = np.arctan2(q[0] @ w, q[0] @ u), np.arctan2(q[1] @ w, q[1] @ u)
        ang = a0 + (1.0 if np.sin(a1 - a0) > 0 else -1.0) * 2.0 * np.pi * np.arange(n) / n
        circle = leg_radius * (np.cos(ang)[:, None] * u + np.sin(ang)[:, None] * w)
        prev = loop
        for r in range(1, rings + 1):
            t = min(r / 4.0, 1.0)
            v.append((1.0 - t) * (p0 + r * step * d) + t * (c + r * step * d + circle))
            ring = list(range(count, count + n))
            count += n
            faces += _strip(prev, ring)
            prev = ring
        legs.append((c, d, 4 * step))
    v = np.concatenate(v)
    if noise:
        v = v + np.random.default_rng(seed).normal(0.0, noise, v.shape)
    return v, np.array(faces, dtype=np.int64), {"seeds": top, "legs": legs, "leg_radius": leg_radius}


def tube_nv(nv):
    """A tube with exactly nv vertices (around a workgroup of 256 and a scan tile of 4096)."""
    return {255: lambda: open_tube(15, 17), 256: lambda: open_tube(16, 16), 257: lambda: wound_tube(15, 17),
            4095: lambda: open_tube(15, 273), 4096: lambda: open_tube(16, 256), 4097: lambda: wound_tube(15, 273)}[nv]()


FIELD_CASES = {
    # name: (mesh, seeds)
    "wound_tube_rim": (lambda: wound_tube(15, 17), list(range(15))),
    "wound_tube_vertex": (lambda: (jitter(wound_tube(15, 17)[0], 4), wound_tube(15, 17)[1]), [100]),
    "open_tube_rim": (lambda: open_tube(), list(range(15))),
    "open_tube_vertex": (lambda: (jitter(open_tube()[0], 5), open_tube()[1]), [254]),
    "two_components": (two_components, [1]),
    "duplicate_seeds": (octahedron, [4, 4, 0, 4]),
    "all_seeded": (octahedron, [5, 4, 3, 2, 1, 0]),
    "isolated_vertex": (with_isolated_vertex, [0]),
    "isolated_seed": (with_isolated_vertex, [6]),
    "one_vertex": (lambda: (np.array([[1.0, 2.0, 3.0]]), np.zeros((0, 3), dtype=np.int64)), [0]),
    "repeated_index": (with_repeated_index, [5]),
    "grid": (grid, [0]),
    "grid_two_seeds": (grid, [0, 168]),
    "nan_vertex": (with_nan_vertex, [20]),
    "strip": (lambda: strip()[:2], [0]),
    "strip_permuted": (lambda: strip(permute_seed=9)[:2], [strip(permute_seed=9)[2]]),
}
FIELD_CASES["trousers"] = (lambda: trousers(noise=0.05, seed=2)[:2], trousers()[2]["seeds"])
for _nv in (255, 256, 257, 4095, 4096, 4097):
    FIELD_CASES[f"tube_nv_{_nv}"] = (functools.partial(tube_nv, _nv), [0, 7])


@functools.lru_cache(maxsize=None)
def field_case(name):
    """(v, f, seeds, dist, pred, report) of the checker, computed once."""
    build, seeds = FIELD_CASES[name]
    v, f = build()
    v, f = np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(f, dtype=np.int64)
    return (v, f, np.array(seeds, dtype=np.int64)) + SK.geodesic(v, f, seeds)


# ---- the checker against itself and scipy ----------------------------------------------------------------------------

HOST_CASES = ("wound_tube_vertex", "open_tube_rim", "two_components", "grid", "nan_vertex", "strip_permuted", "repeated_index",
              "tube_nv_257")


@pytest.mark.parametrize("name", HOST_CASES)
def test_dijkstra_equals_the_jacobi_fixpoint(name):
    v, f, seeds, dist, pred, report = field_case(name)
    e, w, _ = SK.graph_edges(v, f)
    swept, sweeps = SK.jacobi(v.shape[0], e, w, seeds)
    assert same_bits(dist, swept) and sweeps >= 1
    reached = np.isfinite(dist)
    assert report["n_reached"] == reached.sum() and (dist[seeds] == 0).all() and not np.signbit(dist[seeds]).any()
    inner = reached.copy()
    inner[seeds] = False
    assert (pred[inner] >= 0).all() and (pred[~inner] == -1).all()


@pytest.mark.parametrize("name", HOST_CASES)
def test_dijkstra_equals_scipy(name):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import dijkstra
    v, f, seeds, dist, _, _ = field_case(name)
    e, w, _ = SK.graph_edges(v, f)
    nv = v.shape[0]
    keep = w > 0                                                         # a sparse matrix cannot hold an edge of weight 0
    if not keep.all():
        pytest.skip("an edge of length zero")
    g = sp.csr_matrix((np.concatenate([w, w]), (np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]))),
                      shape=(nv, nv))
    assert same_bits(dist, dijkstra(g, directed=True, indices=np.unique(seeds), min_only=True))


def test_the_grid_takes_the_smallest_predecessor():
    v, f, seeds, dist, pred, _ = field_case("grid")
    rows = SK.adjacency(v.shape[0], *SK.graph_edges(v, f)[:2])
    ties = 0
    for i in range(v.shape[0]):
        hits = [u for u, w in rows[i] if dist[u] + w == dist[i]]
        if i != 0:
            assert pred[i] == min(hits)
        ties += len(hits) > 1
    assert ties > 50


def test_skipped_edges_are_counted():
    v, f, seeds, dist, pred, report = field_case("nan_vertex")
    assert report["n_skipped_edges"] > 0 and np.isinf(dist[3]) and pred[3] == -1
    assert report["n_reached"] == v.shape[0] - 1


# ---- Rule T through the C ABI against the checker, on hand-made node graphs -------------------------------------------

def node_graph(rows, edges):
    """rows: (x, y, z, radius, band, flags) per node, in band order"""
    nodes = np.zeros(len(rows), dtype=SK.NODE_DTYPE)
    for n, (x, y, z, r, band, flags) in enumerate(rows):
        nodes[n] = (x, y, z, r, r, 1.0, band, n, 1, flags)
    return nodes, np.array(edges, dtype=np.int64).reshape(-1, 2)


def chain_rows(n, radius=1.0, open_from=None):
    return [(0.7 * k, 0.1 * k * k, 0.0, radius, k, (4 if k == 0 else 0) | (1 if open_from is not None and k >= open_from else 0))
            for k in range(n)]


def _y(arm_b_y=-1.0):
    rows = [(0.0, 0, 0, 0.3, 0, 4), (1.0, 0, 0, 0.3, 1, 0), (2.0, 0, 0, 0.3, 2, 0), (3.0, 1.0, 0, 0.3, 3, 0),
            (3.0, arm_b_y, 0, 0.3, 3, 0), (4.0, 2.0, 0, 0.3, 4, 0), (4.0, 2.0 * arm_b_y, 0, 0.3, 4, 0), (5.0, 3.0, 0, 0.3, 5, 0)]
    return node_graph(rows, [(0, 1), (1, 2), (2, 3), (2, 4), (3, 5), (4, 6), (5, 7)])


def _diamond():
    rows = [(0.0, 0, 0, 1.0, 0, 4), (1.0, 1.0, 0, 1.0, 1, 0), (1.0, -1.0, 0, 1.0, 1, 0), (2.0, 0, 0, 1.0, 2, 0), (3.0, 0, 0, 1.0, 3, 0)]
    return node_graph(rows, [(0, 1), (0, 2), (1, 3), (2, 3), (3, 4)])


def _spurs():
    rows = chain_rows(6) + [(0.9, 0.5, 0.3, 1.0, 2, 0), (2.2, 1.2, 0.4, 1.0, 4, 0)]     # spurs off nodes 1 and 3
    rows = sorted(rows, key=lambda r: r[4])
    # after the sort: 0, 1, 2, spur(band 2), 3, 4, spur(band 4), 5
    return node_graph(rows, [(0, 1), (1, 2), (1, 3), (2, 4), (4, 5), (4, 6), (5, 7)])


def _two_roots():
    rows = [(0.0, 0, 0, 0.5, 0, 4), (0.0, 9.0, 0, 0.5, 0, 4), (1.0, 0, 0, 0.5, 1, 0), (1.0, 9.0, 0, 0.5, 1, 0), (2.0, 0, 0, 0.5, 2, 0),
            (2.0, 9.5, 0, 0.5, 2, 0), (2.0, 8.0, 1.0, 0.5, 2, 0)]
    return node_graph(rows, [(0, 2), (1, 3), (2, 4), (3, 5), (3, 6)])


TERM = lambda x, y, z, r, node: (x, y, z, r, node)                       # noqa: E731
TREE_CASES = {
    # name: (nodes and edges, terminals, min_branch_mm or None)
    "chain": (lambda: node_graph(chain_rows(5), [(k, k + 1) for k in range(4)]), [], None),
    "y": (_y, [], None),
    "y_equal_arms": (lambda: (_y()[0][:7].copy(), np.array([(0, 1), (1, 2), (2, 3), (2, 4), (3, 5), (4, 6)])), [], None),
    "diamond": (_diamond, [], None),
    "diamond_kept_side": (_diamond, [], 0.5),
    "spur_pruned_and_terminal_kept": (_spurs, [TERM(2.3, 1.3, 0.5, 0.4, 6)], None),
    "spurs_all_kept": (_spurs, [], 0.0),
    "open_run_at_a_leaf": (lambda: node_graph(chain_rows(6, open_from=4), [(k, k + 1) for k in range(5)]),
                           [TERM(3.6, 2.6, 0.1, 0.9, 5)], None),
    "open_node_with_a_closed_descendant": (
        lambda: node_graph([r[:5] + (r[5] | (1 if k == 2 else 0),) for k, r in enumerate(chain_rows(5))],
                           [(k, k + 1) for k in range(4)]), [], None),
    "two_roots": (_two_roots, [TERM(2.5, 8.0, 1.5, 0.3, 6)], None),
    "lone_root": (lambda: node_graph([(1.0, 2.0, 3.0, 0.5, 0, 4)], []), [], None),
}


def same_tree(nodes, edges, terminals, min_branch):
    term = np.zeros(len(terminals), dtype=mm.skeleton.TERMINAL_DTYPE)
    for j, t in enumerate(terminals):
        term[j] = t
    cl, rep = mm.skeleton_centerline(nodes, edges, term, min_branch)
    want = SK.tree(nodes, edges, terminals, -1.0 if min_branch is None else min_branch)
    pts = want["points"]
    assert len(cl) == len(pts) and cl.points.dtype == mm.centerline.CL_DTYPE
    for c, name in enumerate(("x", "y", "z", "radius")):
        assert same_bits(cl.points[name], [p[c] for p in pts]), name
    assert cl.points["branch_id"].tolist() == [p[4] for p in pts]
    assert rep["point_node"].tolist() == [p[5] for p in pts]
    tang = np.array(SK.tangents(pts)).reshape(-1, 3)
    for c, name in enumerate(("tx", "ty", "tz")):
        assert same_bits(cl.points[name], tang[:, c]), name
    assert [(b["parent_branch"], b["parent_index"], int(b["ends_at_rim"]), b["n_points"]) for b in rep["branches"]] == want["branches"]
    for k, x in want["report"].items():
        assert rep[k] == x, (k, rep[k], x)
    return cl, rep


@pytest.mark.parametrize("name", sorted(TREE_CASES))
def test_tree_equals_the_checker(name):
    build, terminals, min_branch = TREE_CASES[name]
    nodes, edges = build()
    same_tree(nodes, edges, terminals, min_branch)


def test_tree_cases_show_what_they_are_for():
    run = lambda name: same_tree(*TREE_CASES[name][0](), TREE_CASES[name][1], TREE_CASES[name][2])       # noqa: E731
    cl, rep = run("chain")
    assert rep["n_branches"] == 1 and rep["point_node"].tolist() == [0, 1, 2, 3, 4] and rep["n_loops"] == 0
    cl, rep = run("y")
    assert rep["point_node"].tolist() == [0, 1, 2, 3, 5, 7, 4, 6]           # the side branch starts off its parent
    assert rep["branches"][1] == {"parent_branch": 0, "parent_index": 2, "ends_at_rim": False, "n_points": 2}
    cl, rep = run("y_equal_arms")
    assert rep["point_node"].tolist() == [0, 1, 2, 3, 5, 4, 6]              # equal arms: the smaller leaf is the main vessel
    cl, rep = run("diamond")
    assert rep["n_loops"] == 1 and rep["point_node"].tolist() == [0, 1, 3, 4] and rep["n_pruned"] == 1   # parent of 3 is 1
    cl, rep = run("diamond_kept_side")
    assert rep["point_node"].tolist() == [0, 1, 3, 4, 2] and rep["branches"][1]["parent_index"] == 0
    cl, rep = run("spur_pruned_and_terminal_kept")
    assert rep["n_pruned"] == 1 and 3 not in rep["point_node"] and rep["point_node"].tolist()[-2:] == [6, 8]
    assert rep["branches"][1]["ends_at_rim"] and not rep["branches"][0]["ends_at_rim"]
    cl, rep = run("spurs_all_kept")
    assert rep["n_pruned"] == 0 and rep["n_branches"] == 3
    cl, rep = run("open_run_at_a_leaf")
    assert rep["n_dropped_open"] == 2 and rep["point_node"].tolist() == [0, 1, 2, 3, 6] and rep["branches"][0]["ends_at_rim"]
    cl, rep = run("open_node_with_a_closed_descendant")
    assert rep["n_dropped_open"] == 0 and rep["n_points"] == 5
    cl, rep = run("two_roots")
    assert rep["n_roots"] == 2 and rep["n_components"] == 2 and [b["parent_branch"] for b in rep["branches"]] == [-1, -1, 1]
    assert cl.points["branch_id"].tolist() == [0, 0, 0, 1, 1, 1, 1, 2]
    cl, rep = run("lone_root")
    assert len(cl) == 1 and cl.points["tx"][0] == 0.0


def test_tree_refuses_bad_graphs():
    nodes, edges = TREE_CASES["chain"][0]()
    with pytest.raises(RuntimeError, match="band order"):
        mm.skeleton_centerline(nodes[::-1].copy(), edges)
    with pytest.raises(RuntimeError, match="lo < hi"):
        mm.skeleton_centerline(nodes, edges[:, ::-1].copy())
    with pytest.raises(RuntimeError, match="lo < hi"):
        mm.skeleton_centerline(nodes, [(0, 5)])
    term = np.zeros(1, dtype=mm.skeleton.TERMINAL_DTYPE)
    term["node"] = 5
    with pytest.raises(RuntimeError, match="terminal"):
        mm.skeleton_centerline(nodes, edges, term)
    with pytest.raises(RuntimeError, match="bad arguments"):
        mm.skeleton_centerline(nodes, edges, None, float("nan"))


# ---- the rule's geometry, on the checker ------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [1, 2, 3])
def test_curved_tube_stays_on_the_axis(seed):
    v, f, seeds = curved_tube(seed)
    got = SK.centerline(v, f, seeds)
    pts = np.array([p[:3] for p in got["points"]])
    off = np.hypot(np.hypot(pts[:, 0], pts[:, 1]) - 20.0, pts[:, 2])
    print("curved tube, seed", seed, "points", len(pts), "worst distance from the axis", off.max())
    assert got["report"]["n_branches"] == 1 and got["report"]["n_terminals"] == 1 and got["branches"][0][2] == 1
    assert off.max() <= 0.1 * 2.0


@pytest.mark.parametrize("noise,seed", [(0.0, 0), (0.05, 1), (0.05, 2), (0.05, 3), (0.05, 4)])
def test_trousers_give_two_legs(noise, seed):
    v, f, info = trousers(noise=noise, seed=seed)
    got = SK.centerline(v, f, info["seeds"])
    rep = got["report"]
    assert rep["n_terminals"] == 2 and rep["n_loops"] == 0 and rep["n_branches"] == 2
    assert got["branches"][1][0] == 0 and got["branches"][0][2] == 1 and got["branches"][1][2] == 1
    pts = np.array([p[:3] for p in got["points"]])
    worst, seen = 0.0, 0
    for c, d, s0 in info["legs"]:
        s = (pts - c) @ d
        perp = np.linalg.norm((pts - c) - s[:, None] * d, axis=1)
        mine = (s > s0) & (perp < info["leg_radius"])                     # the points of this leg beyond its blend
        seen += int(mine.sum())
        worst = max(worst, float(perp[mine].max()))
    print("trousers, noise", noise, "seed", seed, "leg points", seen, "worst distance from a leg axis", worst)
    assert seen >= 6 and worst <= 0.1 * info["leg_radius"]


# ---- the public surface ----------------------------------------------------------------------------------------------

def test_public_names():
    for name in ("mesh_geodesic_distance", "mesh_skeleton", "centerline_from_mesh", "skeleton_centerline", "SkeletonGraph"):
        assert name in mm.__all__ and callable(getattr(mm, name))
    p = inspect.signature(mm.mesh_geodesic_distance).parameters
    assert list(p) == ["mesh", "seeds", "engine"] and p["engine"].kind is inspect.Parameter.KEYWORD_ONLY
    assert "lowest index" in mm.mesh_geodesic_distance.__doc__
    p = inspect.signature(mm.mesh_skeleton).parameters
    assert list(p) == ["mesh", "seeds", "band_mm", "engine"] and p["band_mm"].default is None
    assert "isotropic_remesh" in mm.mesh_skeleton.__doc__ and "point_mesh_distance" in mm.mesh_skeleton.__doc__
    p = inspect.signature(mm.centerline_from_mesh).parameters
    assert list(p) == ["mesh", "seeds", "band_mm", "min_branch_mm", "spacing_mm", "smooth_sigma", "engine"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default is None for k in list(p)[2:])
    assert "trim_start" in mm.centerline_from_mesh.__doc__
    assert mm.skeleton.NODE_DTYPE == SK.NODE_DTYPE


def test_sources_are_built():
    from multimoda_rs_amd import build as b
    assert "mm_geodesic_kernels.hip" in b.SOURCES and "mm_geodesic.cpp" in b.SOURCES and "-ffp-contract=off" in b.FLAGS


def test_bad_arguments_are_refused_before_the_device():
    v, f = octahedron()
    for seeds in ([], [6], [-1], [0.5], [[0.0, 0.0]], "x"):
        with pytest.raises(ValueError):
            mm.mesh_geodesic_distance((v, f), seeds)
    with pytest.raises(ValueError):
        mm.mesh_geodesic_distance((v, f + 1), [0])
    with pytest.raises(ValueError):
        mm.mesh_geodesic_distance((np.full((6, 3), np.nan), f), np.array([0.0, 0.0, 0.0]))
    for band in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            mm.mesh_skeleton((v, f), [0], band_mm=band)
        with pytest.raises(ValueError):
            mm.centerline_from_mesh((v, f), [0], band_mm=band)
    with pytest.raises(ValueError):
        mm.centerline_from_mesh((v, f), [0], min_branch_mm=-0.5)
    with pytest.raises(ValueError):
        mm.mesh_skeleton((v[:1], f[:0]), [0])                              # no edge: no default band


def test_a_seed_point_means_the_nearest_vertex_lowest_index_first():
    from multimoda_rs_amd import skeleton
    v, _ = octahedron()
    assert skeleton._seed_vertices(np.array([0.9, 0.1, 0.0]), v).tolist() == [0]
    assert skeleton._seed_vertices(np.array([0.0, 0.0, 0.0]), v).tolist() == [0]        # all six are as near
    assert skeleton._seed_vertices(np.array([0.0, 0.5, 0.5]), v).tolist() == [2]        # 2 and 4 tie
    assert skeleton._seed_vertices([3, 3, 1], v).tolist() == [3, 3, 1]
