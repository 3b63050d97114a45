"""Rules G and S of include/mm_centerline.h on the worst cases of tests/geo_attack_cases.py, without a device: the rule as
tests/mm_checkers/mesh_skeleton.py restates it against tests/geo_exact.py, an oracle in rational arithmetic and a plain
breadth-first search that share no code with it.  tests/test_gpu_geo_attack.py runs the same checks (check_field,
check_partition) on what the device returns.

Every case first shows what it is for, on the checker's output: the rank and block of the hub's predecessor; the hub
that falls a second time and the block only it can flag; the vertices of a detour that fall three times or more under
synchronous sweeps; the edges skipped, the vertices reached and the zeros of the weight cases; the node and node-edge
counts and the flag bits of the band cases.

Then (G) the checker's field lies within the derived bound of the exact field (field_bound: D (1 -+ u)^(nv - 1), u = 2^-53)
and its predecessors satisfy the definition re-derived in check_pred, and (S) the checker's partition, numbering,
vertex_node, first_vertex, n_vertices and node edges equal components_by_band of its own dist.

The claim of an overflowing path sum cannot be staged from a mesh: a finite weight is a square root of a finite double,
below 2^512, and fewer than 2^31 of them stay far below 2^1024 (weights_overflow_sum_strip pins that every connected vertex
is reached at the largest weights there are).  test_rounded_sums_that_overflow runs the checker's Dijkstra on weights
given directly instead, where a connected vertex does stay at +inf, and the oracle allows exactly that.

Worst |dist - D| / (D u) measured on the checker (test_field_within_the_bound_of_the_exact_field prints each; the bound
is about nv - 1, 599 to 1101 here): hub_ at most 25.6, detour_ 1.32, weights_ at most 7.8."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import geo_attack_cases as AC
import geo_exact as EX
from mm_checkers import mesh_skeleton as SK

HUB_NAMES = tuple(n for n in AC.NAMES if AC.family(n) == "hub")
DETOUR_NAMES = tuple(n for n in AC.NAMES if AC.family(n) == "detour")
WEIGHTS_NAMES = tuple(n for n in AC.NAMES if AC.family(n) == "weights")


@functools.lru_cache(maxsize=None)
def graph(name):
    """(edges as a list of pairs, weights as a list of floats, rows, n_skipped) of a case, by the checker's graph_edges."""
    _, v, f = AC.cases()[name][:3]
    e, w, skipped = SK.graph_edges(v, f)
    return e.tolist(), w.tolist(), SK.adjacency(len(v), e, w), skipped


@functools.lru_cache(maxsize=None)
def checked(name):
    """The checker's (dist, pred, report) of a field case, computed once for both files."""
    _, v, f, seeds = AC.cases()[name][:4]
    return SK.geodesic(v, f, seeds)


@functools.lru_cache(maxsize=None)
def exact(name):
    _, v, f, seeds = AC.cases()[name][:4]
    e, w, _, _ = graph(name)
    return EX.exact_field(len(v), e, w, seeds.tolist())


def check_field(name, dist, pred):
    """(G) on any dist and pred offered for the case; returns the worst ratio to D u."""
    _, v, f, seeds = AC.cases()[name][:4]
    D, _ = exact(name)
    worst = EX.field_bound(dist, D, len(v))
    EX.check_pred(graph(name)[2], dist, pred, seeds.tolist())
    return worst


def band_index(dist, h):
    """Rule S: (int64)(dist / h) from one f64 division, -1 where dist is +inf."""
    return [int(float(x) / float(h)) if math.isfinite(x) else -1 for x in np.asarray(dist, dtype=np.float64).tolist()]


def check_partition(name, dist, vertex_node, nodes, edges):
    """(S) on any skeleton offered for the case, against components_by_band of the dist that came with it."""
    _, v, f, seeds, h = AC.cases()[name]
    e, w, _, _ = graph(name)
    want_node, want_nodes, want_edges = EX.components_by_band(len(v), e, w, band_index(dist, h))
    assert np.asarray(vertex_node).tolist() == want_node
    assert len(nodes) == len(want_nodes)
    assert [(int(n["band"]), int(n["first_vertex"]), int(n["n_vertices"])) for n in nodes] == want_nodes
    assert [tuple(p) for p in np.asarray(edges).reshape(-1, 2).tolist()] == want_edges
    return len(want_nodes), len(want_edges)


@functools.lru_cache(maxsize=None)
def skeleton_checked(name):
    _, v, f, seeds, h = AC.cases()[name]
    return SK.skeleton(v, f, seeds, h)


# ---- every case shows what it is for ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", HUB_NAMES)
def test_hub_cases_are_what_they_say(name):
    _, v, f, seeds = AC.cases()[name]
    d, hub, kind = AC.hub_of(name)
    rows = graph(name)[2]
    dist, pred, rep = checked(name)
    row = [u for u, _ in rows[hub]]
    assert len(v) == AC.NV_HUB and rep["n_reached"] == len(v) and rep["n_skipped_edges"] == 0
    assert row == AC.hub_ring(d, hub) and len(row) == d
    assert len({AC.block_of(u) for u in row}) >= 2
    if kind in ("early_out", "late_out", "late_in"):
        rank = row.index(int(pred[hub]))
        assert rank == AC.hub_entry_rank(d, hub, kind)
        assert (rank >= AC.ROW) == kind.startswith("late")
        assert (AC.block_of(row[rank]) == AC.block_of(hub)) == kind.endswith("in")
        # only the entry's two ring neighbours take their value along the ring: the rest of the ring hangs on the hub
        assert sum(int(pred[u]) == hub for u in row) == d - 3
        print(f"{name}: the hub's predecessor {row[rank]} is entry {rank} of {d}, block {AC.block_of(row[rank])}; the hub in "
              f"block {AC.block_of(hub)}")
    elif kind == "seed":
        assert seeds.tolist() == [hub] and dist[hub] == 0.0 and all(int(pred[u]) == hub for u in row)
        print(f"{name}: the seed's row of {d} lies in blocks {sorted({AC.block_of(u) for u in row})}")
    else:
        x, sequence, (a1, a2), b = AC.hub_meet_plan(d, hub)
        alone, _, _ = SK.geodesic(v, f, seeds[:1])                        # strip A's seed alone: the field before B arrives
        assert int(pred[hub]) == row[b] and 0.009 < alone[hub] - dist[hub] < 0.011
        assert all(AC.block_of(u) != x for u in row[:AC.ROW]) and AC.block_of(hub) != x
        arc = [u for u in row if AC.block_of(u) == x]
        assert arc and all(row.index(u) >= AC.ROW for u in arc)
        for u in arc:                                                    # falls with the hub, and no neighbour in another block does
            assert int(pred[u]) == hub and dist[u] < alone[u]
            for t, _ in rows[u]:
                assert t == hub or AC.block_of(t) == x or dist[t] == alone[t], (u, t)
        late = [i for i in range(len(v)) if AC.block_of(i) == x and dist[i] < alone[i]]
        assert sorted(late) == sorted(arc)                               # nothing else of X falls late: only the hub can flag it
        print(f"{name}: the hub falls again by {alone[hub] - dist[hub]:.6f}; block {x} holds {len(arc)} ring vertices that fall with it "
              f"and none of the hub's first {AC.ROW} entries")


def fall_counts(nv, edges, weights, seeds):
    """Synchronous sweeps as SK.jacobi: (how often every vertex fell, the sweeps)."""
    e, w = np.array(edges, dtype=np.int64).reshape(-1, 2), np.array(weights, dtype=np.float64)
    dist = np.full(nv, np.inf)
    dist[np.asarray(seeds, dtype=np.int64)] = 0.0
    falls, sweeps = np.zeros(nv, dtype=np.int64), 0
    while True:
        new = dist.copy()
        np.minimum.at(new, e[:, 1], dist[e[:, 0]] + w)
        np.minimum.at(new, e[:, 0], dist[e[:, 1]] + w)
        sweeps += 1
        if np.array_equal(new, dist):
            return falls, sweeps, dist
        falls += new < dist
        dist = new


@pytest.mark.parametrize("name", DETOUR_NAMES)
def test_detour_vertices_fall_again_and_again(name):
    _, v, f, seeds = AC.cases()[name]
    e, w, rows, _ = graph(name)
    falls, sweeps, swept = fall_counts(len(v), e, w, seeds.tolist())
    dist, _, _ = checked(name)
    assert np.array_equal(swept.view(np.uint64), dist.view(np.uint64))
    assert all(u != int(seeds[0]) for i in range(len(v)) if v[i, 2] == 0.0 and i != int(seeds[0]) for u, _ in rows[i])
    across = sum(AC.block_of(a) != AC.block_of(b) for a, b in e)
    print(f"{name}: nv {len(v)}, {int((falls >= 3).sum())} vertices fall three times or more (at most {int(falls.max())}), "
          f"{sweeps} sweeps; {across} of {len(e)} edges cross blocks; the seed's valence {len(rows[int(seeds[0])])}")
    assert int((falls >= 3).sum()) >= 100
    blocks = -(-len(v) // AC.BLOCK)
    assert blocks == {"detour_2_blocks": 2, "detour_3_blocks": 3, "detour_5_blocks": 5, "detour_in_order": 3}[name]
    if name != "detour_in_order":
        assert across > 0.4 * len(e)


@pytest.mark.parametrize("name", WEIGHTS_NAMES)
def test_weight_cases_are_what_they_say(name):
    _, v, f, seeds = AC.cases()[name]
    e, w, rows, skipped = graph(name)
    dist, pred, rep = checked(name)
    nv = len(v)
    w = np.array(w)
    span = math.log2(w[w > 0].max() / w[w > 0].min()) if (w > 0).any() else 0.0
    print(f"{name}: {len(e)} edges, {skipped} skipped, {rep['n_reached']} of {nv} reached; weights over {span:.1f} binades, "
          f"{int((w == 0).sum())} zero")
    if "scales" in name:
        assert skipped == 0 and rep["n_reached"] == nv and span > 40
    elif "2m520" in name:
        assert skipped == 0 and rep["n_reached"] == nv and (w > 0).all()
        with np.errstate(under="ignore"):
            assert (w * w < 2.0 ** -1022).all()                           # every square is subnormal
    elif "2m600" in name:
        assert skipped == 0 and rep["n_reached"] == nv and (w == 0).all()
        assert (dist.view(np.uint64) == 0).all() and rep["max_dist"] == 0.0
        mutual = [(a, int(pred[a])) for a in range(nv) if pred[a] >= 0 and pred[pred[a]] == a]
        assert any(AC.block_of(a) != AC.block_of(b) for a, b in mutual)   # each other's predecessor, across blocks
    elif "2p500" in name:
        assert skipped == 0 and rep["n_reached"] == nv and w.min() > 2.0 ** 495
    elif "overflow_some" in name:
        assert skipped == 2 * len(AC.LIFTED_PARTLY) + 6 * len(AC.LIFTED_OFF) and rep["n_skipped_edges"] == skipped
        off = [r * 25 + c for r, c in AC.LIFTED_OFF]
        assert rep["n_reached"] == nv - len(off) and np.isinf(dist[off]).all()
        assert np.isfinite(dist[[r * 25 + c for r, c in AC.LIFTED_PARTLY]]).all()
    elif "overflow_sum" in name:
        # the largest weights the rule can produce: still every connected vertex is reached (the module's docstring)
        assert skipped == 0 and w.max() < 2.0 ** 512 and w.min() > 2.0 ** 511
        component = EX.components_by_band(nv, e, w.tolist(), [0] * nv)[1]
        assert len(component) == 1 and component[0][2] == nv == rep["n_reached"]
        assert np.isfinite(dist).all() and rep["max_dist"] > 2.0 ** 519
    elif "duplicates" in name:
        assert skipped == 0 and rep["n_reached"] == nv and int((w == 0).sum()) == 2
        for a, b in AC.DUPLICATES[:2]:
            assert AC.block_of(a) != AC.block_of(b) and dist[a] == dist[b] and b in [u for u, _ in rows[a]]
    else:
        assert skipped == 12 and rep["n_reached"] == nv - 2
        assert np.isinf(dist[[AC.NAN_VERTEX, AC.INF_VERTEX]]).all() and pred[AC.NAN_VERTEX] == -1 == pred[AC.INF_VERTEX]
        assert AC.block_of(AC.NAN_VERTEX - 25) == 0 and AC.block_of(AC.NAN_VERTEX) == 1
        assert AC.block_of(AC.INF_VERTEX + 25) == 2 and AC.block_of(AC.INF_VERTEX) == 1


@pytest.mark.parametrize("name", AC.BANDS_NAMES)
def test_band_cases_are_what_they_say(name):
    _, v, f, seeds, h = AC.cases()[name]
    sk = skeleton_checked(name)
    nodes, edges = sk["nodes"], sk["edges"]
    print(f"{name}: nv {len(v)}, band {h}: {len(nodes)} nodes, {len(edges)} node edges, flags {sorted(set(nodes['flags'].tolist()))}")
    if name in AC.BANDS_EXPECT:
        assert (len(nodes), len(edges)) == AC.BANDS_EXPECT[name]
    if (name.startswith("bands_nodes_") and h == 1.0) or name in ("bands_half_65", "bands_three_768"):
        on_boundary = sum(Fraction(float(x)) % Fraction(h) == 0 for x in sk["dist"])
        assert on_boundary >= (len(v) // 2 if h <= 1.0 else len(v) // 6)   # the bottom row sits on the band boundaries
    if name == "bands_tenth_30":
        exact_band = [math.floor(Fraction(float(x)) / Fraction(h)) for x in sk["dist"]]
        assert sum(a != b for a, b in zip(exact_band, band_index(sk["dist"], h))) > 0   # the rounded quotient decides
    if name in ("bands_hub_one_node", "bands_one_band_permuted"):
        assert nodes["n_vertices"][0] == len(v) and len(f) * 3 >= 1500                   # one lane walks them all
    if name == "bands_one_band_permuted":
        assert len(v) >= 2000
    if name == "bands_two_fat":
        e = graph(name)[0]
        joining = sum(sk["vertex_node"][a] != sk["vertex_node"][b] for a, b in e)
        assert joining >= 200 and nodes["n_vertices"].tolist() == [300, 300]
        print(f"{name}: {joining} edges of the graph join the two nodes")
    if name == "bands_plain_mean":
        plain = nodes[(nodes["flags"] & 2) != 0]
        assert len(plain) == 5 and (plain["first_vertex"] >= AC.BLOCK).all() and len(v) > 3 * AC.BLOCK
        assert sorted(plain["first_vertex"].tolist()) == [299, 300, 301, 800, 801]
        assert (plain["weight"] == 0.0).all() and np.isfinite(plain["x"]).all()
        assert sk["vertex_node"][AC.PLAIN_N + AC.PLAIN_NAN] == -1


def test_the_sort_sizes_are_met():
    counts = [AC.BANDS_EXPECT[n] for n in AC.BANDS_NAMES if n in AC.BANDS_EXPECT]
    assert {1, 2, 3, 4, 5, 255, 256, 257, 4096, 4097} <= {k for k, _ in counts}
    assert {256, 257, 4096} <= {m for _, m in counts}


# ---- (G) and (S): the checker against the exact oracle --------------------------------------------------------------------

@pytest.mark.parametrize("name", AC.FIELD_NAMES)
def test_field_within_the_bound_of_the_exact_field(name):
    dist, pred, _ = checked(name)
    worst = check_field(name, dist, pred)
    _, hops = exact(name)
    print(f"{name}: worst |dist - D| / (D u) = {worst:.2f} of at most about {len(dist) - 1}; an exact shortest path has up to "
          f"{max(hops)} hops")


@pytest.mark.parametrize("name", AC.BANDS_NAMES)
def test_partition_equals_the_breadth_first_search(name):
    sk = skeleton_checked(name)
    k, m = check_partition(name, sk["dist"], sk["vertex_node"], sk["nodes"], sk["edges"])
    assert (k, m) == (sk["report"]["n_nodes"], sk["report"]["n_node_edges"])


# ---- the oracle is no rubber stamp -----------------------------------------------------------------------------------------

def test_rounded_sums_that_overflow():
    """A chain of weights 2^1023 and a side door of 2^1022: vertex 2 is connected, its only rounded sum is 2^1024 = +inf,
    so it stays unreached, and field_bound allows that only because D (1 + u)^(nv - 1) reaches the overflow threshold."""
    edges, weights = [(0, 1), (1, 2), (0, 3)], [2.0 ** 1023, 2.0 ** 1023, 2.0 ** 1022]
    rows = SK.adjacency(4, np.array(edges), np.array(weights))
    dist = SK.dijkstra(4, rows, [0])
    assert dist.tolist() == [0.0, 2.0 ** 1023, math.inf, 2.0 ** 1022]
    D, hops = EX.exact_field(4, edges, weights, [0])
    assert D[2] == 2 ** 1024 and hops == [0, 1, 2, 1]
    EX.field_bound(dist, D, 4)
    pred = SK.predecessors(rows, dist, [0])
    assert pred.tolist() == [-1, 0, -1, 0]
    EX.check_pred(rows, dist, pred, [0])
    wrong = dist.copy()
    wrong[3] = math.inf                                                  # 2^1022 cannot overflow: +inf is refused there
    with pytest.raises(AssertionError):
        EX.field_bound(wrong, D, 4)


def test_the_oracle_refuses_a_wrong_field():
    name = "hub_late_out_300_599"
    dist, pred, _ = checked(name)
    _, hub, _ = AC.hub_of(name)
    D, _ = exact(name)
    for factor in (1.0 + 2.0 ** -40, 1.0 - 2.0 ** -40):                    # 8192 u: past the bound of 599 u, far below any eye
        wrong = dist.copy()
        wrong[hub] *= factor
        with pytest.raises(AssertionError):
            EX.field_bound(wrong, D, len(dist))
    wrong = dist.copy()
    wrong[dist == 0.0] = -0.0
    with pytest.raises(AssertionError):
        EX.field_bound(wrong, D, len(dist))
    rows, seeds = graph(name)[2], AC.cases()[name][3].tolist()
    for v, p in ((hub, -1), (hub, rows[hub][0][0]), (seeds[0], rows[seeds[0]][0][0])):
        wrong = pred.copy()
        wrong[v] = p
        with pytest.raises(AssertionError):
            EX.check_pred(rows, dist, wrong, seeds)


def test_the_search_refuses_a_wrong_partition():
    name = "bands_nodes_5"
    sk = skeleton_checked(name)
    check_partition(name, sk["dist"], sk["vertex_node"], sk["nodes"], sk["edges"])
    merged = sk["vertex_node"].copy()
    merged[merged == 4] = 3
    with pytest.raises(AssertionError):
        check_partition(name, sk["dist"], merged, sk["nodes"], sk["edges"])
    with pytest.raises(AssertionError):
        check_partition(name, sk["dist"], sk["vertex_node"], sk["nodes"], sk["edges"][:-1])
    with pytest.raises(AssertionError):
        check_partition(name, sk["dist"], sk["vertex_node"], sk["nodes"][::-1], sk["edges"])
