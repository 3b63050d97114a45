"""An oracle for rules G and S of include/mm_centerline.h in exact arithmetic: plain Python, fractions.Fraction and
integers, no numpy arithmetic on a value, and no code shared with tests/mm_checkers/mesh_skeleton.py or the C++.

The weights are taken as given (the f64 numbers rule G computes): what is checked is the claim about the sums.

field_bound's bound is derived, not measured.  A rounded addition returns (a + b)(1 + e) with |e| <= u = 2^-53 (a sum in
the subnormal range is exact), so a path's sum rounded after every addition lies within (1 - u)^hops and (1 + u)^hops of
its exact sum.  dist[v] is the minimum of the rounded sums over the paths, so it is at least D (1 - u)^(nv - 1) -- every
path's exact sum is at least D and no simple path has more than nv - 1 edges, and a walk that repeats a vertex is no
shorter than the path inside it, rounded or not, as rounded addition is monotone -- and at most the rounded sum along an
exact shortest path, D (1 + u)^(nv - 1).  Where that is below the overflow threshold 2^1024 - 2^970 the rounded sum along
that path is finite, so dist[v] is."""
import heapq
from fractions import Fraction

U = Fraction(1, 2 ** 53)
OVERFLOW = Fraction(2 ** 1024 - 2 ** 970)
INF = float("inf")


def exact_field(nv, edges, weights, seeds):
    """Dijkstra over Fractions: (D, hops), D[v] the exact distance or None, hops[v] the edges of one exact shortest path.
    edges [(a, b)], weights the f64 of each; an edge whose weight is not finite is left out."""
    rows = [[] for _ in range(nv)]
    for (a, b), w in zip(edges, weights):
        w = float(w)
        if w != w or w in (INF, -INF):
            continue
        q = Fraction(w)
        assert q >= 0
        rows[int(a)].append((int(b), q))
        rows[int(b)].append((int(a), q))
    D, hops, heap = [None] * nv, [0] * nv, []
    for s in sorted(set(int(s) for s in seeds)):
        D[s] = Fraction(0)
        heap.append((Fraction(0), s))
    heapq.heapify(heap)
    done = [False] * nv
    while heap:
        d, x = heapq.heappop(heap)
        if done[x]:
            continue
        done[x] = True
        for t, w in rows[x]:
            c = d + w
            if D[t] is None or c < D[t]:
                D[t], hops[t] = c, hops[x] + 1
                heapq.heappush(heap, (c, t))
    return D, hops


def field_bound(dist, D, nv):
    """Asserts dist against the exact field D; returns the worst |dist - D| / (D u) over the vertices with D > 0."""
    lo, hi = (1 - U) ** max(nv - 1, 0), (1 + U) ** max(nv - 1, 0)
    worst = Fraction(0)
    for v in range(nv):
        x = float(dist[v])
        if D[v] is None:
            assert x == INF, (v, x, "no path arrives")
            continue
        if x == INF:
            assert D[v] * hi >= OVERFLOW, (v, "a finite exact distance whose rounded sum cannot overflow, and +inf")
            continue
        assert x == x and x >= 0.0 and x != INF, (v, x)
        if D[v] == 0:
            assert x == 0.0 and str(x) == "0.0", (v, x, "exact distance 0")
            continue
        q = Fraction(x)
        assert D[v] * lo <= q <= D[v] * hi, (v, x, float(D[v]))
        worst = max(worst, abs(q - D[v]) / (D[v] * U))
    return float(worst)


def check_pred(rows, dist, pred, seeds):
    """pred from its definition: -1 exactly at the seeds and where dist is +inf; elsewhere the smallest neighbour u with
    fl(dist[u] + w) == dist[v], which every reached vertex that is no seed has.  rows[v] = [(u, w)], any order."""
    seeds = set(int(s) for s in seeds)
    for v in range(len(rows)):
        x, p = float(dist[v]), int(pred[v])
        if v in seeds or x == INF:
            assert p == -1, (v, p)
            continue
        fit = [int(u) for u, w in rows[v] if float(dist[u]) + float(w) == x]
        assert fit, (v, x, "no neighbour gives this distance")
        assert p == min(fit), (v, p, min(fit))


def components_by_band(nv, edges, weights, band_index):
    """Rule S's partition by a breadth-first search: (vertex_node, nodes, node_edges).  band_index[v] < 0 = in no band.
    nodes = [(band, first_vertex, n_vertices)] in the order (band, smallest vertex); node_edges = the sorted pairs (lo, hi)
    of different nodes that an edge of finite weight joins."""
    rows = [[] for _ in range(nv)]
    kept = []
    for (a, b), w in zip(edges, weights):
        w = float(w)
        if w != w or w in (INF, -INF):
            continue
        rows[int(a)].append(int(b))
        rows[int(b)].append(int(a))
        kept.append((int(a), int(b)))
    label = [-1] * nv
    found = []
    for s in range(nv):                                                  # ascending: a component is found at its smallest vertex
        if band_index[s] < 0 or label[s] >= 0:
            continue
        label[s] = len(found)
        queue, size = [s], 0
        while queue:
            x = queue.pop()
            size += 1
            for t in rows[x]:
                if label[t] < 0 and band_index[t] == band_index[s]:
                    label[t] = label[s]
                    queue.append(t)
        found.append((int(band_index[s]), s, size))
    order = sorted(range(len(found)), key=lambda i: found[i][:2])
    number = {old: new for new, old in enumerate(order)}
    vertex_node = [number[label[v]] if label[v] >= 0 else -1 for v in range(nv)]
    pairs = set()
    for a, b in kept:
        na, nb = vertex_node[a], vertex_node[b]
        if na >= 0 and nb >= 0 and na != nb:
            pairs.add((min(na, nb), max(na, nb)))
    return vertex_node, [found[i] for i in order], sorted(pairs)
