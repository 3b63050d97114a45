"""Independent restatement of the centerline-from-mesh rules (include/mm_centerline.h, rules G, S and T) in numpy and
heapq, sharing no code with the C++.  Every operation is written in the order the rule states; numpy's f64 arithmetic is
IEEE and unfused, so the results are comparable bit for bit."""
import heapq
import math

import numpy as np


# ---- Rule G: the field ------------------------------------------------------------------------------------------------

def graph_edges(vertices, faces):
    """(edges int64[m, 2] with lo < hi, sorted; weights f64[m]; n_skipped): the distinct undirected edges of the faces
    between different vertices whose weight is finite."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    pairs = set()
    for a, b, c in f.tolist():
        for p, q in ((a, b), (b, c), (c, a)):
            if p != q:
                pairs.add((min(p, q), max(p, q)))
    e = np.array(sorted(pairs), dtype=np.int64).reshape(-1, 2)
    with np.errstate(all="ignore"):
        d = v[e[:, 1]] - v[e[:, 0]]
        w = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    keep = np.isfinite(w)
    return e[keep], w[keep], int((~keep).sum())


def adjacency(nv, edges, weights):
    """rows[v] = [(u, w)] ascending in u."""
    rows = [[] for _ in range(nv)]
    for (a, b), w in zip(edges.tolist(), weights.tolist()):
        rows[a].append((b, w))
        rows[b].append((a, w))
    for r in rows:
        r.sort()
    return rows


def dijkstra(nv, rows, seeds):
    """Heap Dijkstra with rounded left-to-right sums: dist f64[nv], +inf where no path arrives."""
    dist = [float("inf")] * nv
    heap = []
    for s in sorted(set(int(s) for s in seeds)):
        dist[s] = 0.0
        heap.append((0.0, s))
    heapq.heapify(heap)
    done = [False] * nv
    while heap:
        d, u = heapq.heappop(heap)
        if done[u]:
            continue
        done[u] = True
        for t, w in rows[u]:
            c = d + w
            if c < dist[t]:
                dist[t] = c
                heapq.heappush(heap, (c, t))
    return np.array(dist, dtype=np.float64)


def jacobi(nv, edges, weights, seeds):
    """Full sweeps of d[v] = min(d[v], d[u] + w) over all edges at once until nothing falls: (dist, sweeps)."""
    dist = np.full(nv, np.inf)
    dist[np.asarray(list(seeds), dtype=np.int64)] = 0.0
    a, b = edges[:, 0], edges[:, 1]
    sweeps = 0
    while True:
        new = dist.copy()
        np.minimum.at(new, b, dist[a] + weights)
        np.minimum.at(new, a, dist[b] + weights)
        sweeps += 1
        if np.array_equal(new, dist):
            return dist, sweeps
        dist = new


def predecessors(rows, dist, seeds):
    nv = len(rows)
    is_seed = np.zeros(nv, dtype=bool)
    is_seed[np.asarray(list(seeds), dtype=np.int64)] = True
    pred = np.full(nv, -1, dtype=np.int64)
    for v in range(nv):
        if is_seed[v] or not np.isfinite(dist[v]):
            continue
        for u, w in rows[v]:
            if dist[u] + w == dist[v]:
                pred[v] = u
                break
    return pred


def geodesic(vertices, faces, seeds):
    """(dist, pred, report) of Rule G; report holds the counts that are a function of the input."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    nv = v.shape[0]
    e, w, skipped = graph_edges(v, faces)
    rows = adjacency(nv, e, w)
    dist = dijkstra(nv, rows, seeds)
    pred = predecessors(rows, dist, seeds)
    finite = np.isfinite(dist)
    report = {"n_vertices": nv, "n_faces": int(np.asarray(faces).reshape(-1, 3).shape[0]), "n_edges": int(e.shape[0]),
              "n_skipped_edges": skipped, "n_reached": int(finite.sum()),
              "max_dist": float(dist[finite].max()) if finite.any() else 0.0,
              "max_edge": float(w.max()) if w.size else 0.0}
    return dist, pred, report


GEODESIC_COUNTS = ("n_vertices", "n_faces", "n_edges", "n_skipped_edges", "n_reached", "max_dist", "max_edge")


# ---- Rule S: the nodes -----------------------------------------------------------------------------------------------

NODE_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("radius", "<f8"), ("radius_min", "<f8"), ("weight", "<f8"),
                       ("band", "<i8"), ("first_vertex", "<i8"), ("n_vertices", "<i8"), ("flags", "<i8")])


def _norm(dx, dy, dz):
    return math.sqrt((dx * dx + dy * dy) + dz * dz)


def rim_vertices(nv, faces):
    """The ends of the edges {lo < hi} that exactly one corner of one face spans."""
    count = {}
    for a, b, c in np.asarray(faces, dtype=np.int64).reshape(-1, 3).tolist():
        for p, q in ((a, b), (b, c), (c, a)):
            if p != q:
                k = (min(p, q), max(p, q))
                count[k] = count.get(k, 0) + 1
    rim = np.zeros(nv, dtype=bool)
    for (p, q), n in count.items():
        if n == 1:
            rim[p] = rim[q] = True
    return rim


def skeleton(vertices, faces, seeds, h):
    """Rule S: dict(dist, pred, vertex_node, nodes (NODE_DTYPE), edges int64[m, 2], report)."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    nv = v.shape[0]
    h = float(h)
    dist, pred, report = geodesic(v, f, seeds)
    e, _, _ = graph_edges(v, f)
    band = np.full(nv, -1, dtype=np.int64)
    for i in range(nv):
        if math.isfinite(dist[i]):
            q = float(dist[i]) / h
            if q >= 2147483648.0:
                raise OverflowError("a band index passes 2^31")
            band[i] = int(q)
    root = list(range(nv))

    def find(x):
        while root[x] != x:
            root[x] = root[root[x]]
            x = root[x]
        return x

    for a, b in e.tolist():
        if band[a] >= 0 and band[a] == band[b]:
            ra, rb = find(a), find(b)
            if ra != rb:
                root[max(ra, rb)] = min(ra, rb)
    reps = sorted({(int(band[i]), find(i)) for i in range(nv) if band[i] >= 0})
    number = {r: n for n, (_, r) in enumerate(reps)}
    vnode = np.array([number[find(i)] if band[i] >= 0 else -1 for i in range(nv)], dtype=np.int64)
    k = len(reps)
    members = [[] for _ in range(k)]
    for i in range(nv):
        if vnode[i] >= 0:
            members[vnode[i]].append(i)
    # the area-weighted sums, face by face, corner by corner
    with np.errstate(all="ignore"):
        e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        a3 = (0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)) / 3.0
    a3 = a3.tolist()
    vl, fl = v.tolist(), f.tolist()
    W, S, bad = [0.0] * k, [[0.0, 0.0, 0.0] for _ in range(k)], [False] * k
    for t, corners in enumerate(fl):
        for p in corners:
            n = vnode[p]
            if n < 0:
                continue
            a = a3[t]
            bad[n] = bad[n] or not math.isfinite(a)
            W[n] = W[n] + a
            for c in range(3):
                S[n][c] = S[n][c] + a * vl[p][c]
    plain = [bad[n] or not (W[n] > 0.0) for n in range(k)]
    centre = []
    for n in range(k):
        if plain[n]:
            s = [0.0, 0.0, 0.0]
            for p in members[n]:
                for c in range(3):
                    s[c] = s[c] + vl[p][c]
            div = float(len(members[n]))
        else:
            s, div = S[n], W[n]
        with np.errstate(all="ignore"):
            centre.append([float(np.float64(s[c]) / np.float64(div)) for c in range(3)])
    R = [0.0] * k
    for t, corners in enumerate(fl):
        for p in corners:
            n = vnode[p]
            if n >= 0 and not plain[n]:
                R[n] = R[n] + a3[t] * _norm(vl[p][0] - centre[n][0], vl[p][1] - centre[n][1], vl[p][2] - centre[n][2])
    rim = rim_vertices(nv, f)
    is_seed = np.zeros(nv, dtype=bool)
    is_seed[np.asarray(list(seeds), dtype=np.int64)] = True
    nodes = np.zeros(k, dtype=NODE_DTYPE)
    for n in range(k):
        least = math.inf
        for p in members[n]:
            r = _norm(vl[p][0] - centre[n][0], vl[p][1] - centre[n][1], vl[p][2] - centre[n][2])
            if plain[n]:
                R[n] = R[n] + r
            if r < least:
                least = r
        flags = 2 if plain[n] else 0
        if any(rim[p] and not is_seed[p] for p in members[n]):
            flags |= 1
        if any(is_seed[p] for p in members[n]):
            flags |= 4
        with np.errstate(all="ignore"):
            radius = float(np.float64(R[n]) / np.float64(float(len(members[n])) if plain[n] else W[n]))
        nodes[n] = (centre[n][0], centre[n][1], centre[n][2], radius, least, 0.0 if plain[n] else W[n], reps[n][0],
                    members[n][0], len(members[n]), flags)
    pairs = sorted({(min(vnode[a], vnode[b]), max(vnode[a], vnode[b])) for a, b in e.tolist()
                    if vnode[a] >= 0 and vnode[b] >= 0 and vnode[a] != vnode[b]})
    edges = np.array(pairs, dtype=np.int64).reshape(-1, 2)
    report = dict(report, n_nodes=k, n_node_edges=int(edges.shape[0]))
    return {"dist": dist, "pred": pred, "vertex_node": vnode, "nodes": nodes, "edges": edges, "report": report}


def default_band(vertices, faces):
    """Twice the longest finite edge."""
    w = graph_edges(vertices, faces)[1]
    return 2.0 * float(w.max())


# ---- Rule T: terminals, tree, branches -------------------------------------------------------------------------------

def rim_loops(nv, faces):
    """The rim loops as vertex lists, each starting at its smallest vertex and going on to the smaller of that vertex's two
    rim neighbours; loops in ascending order of their smallest vertex.  Every rim vertex must have two rim neighbours."""
    count = {}
    for a, b, c in np.asarray(faces, dtype=np.int64).reshape(-1, 3).tolist():
        for p, q in ((a, b), (b, c), (c, a)):
            if p != q:
                k = (min(p, q), max(p, q))
                count[k] = count.get(k, 0) + 1
    nbr = {}
    for (p, q), n in count.items():
        if n == 1:
            nbr.setdefault(p, []).append(q)
            nbr.setdefault(q, []).append(p)
    assert all(len(x) == 2 for x in nbr.values()), "an irregular rim"
    seen, loops = set(), []
    for start in sorted(nbr):
        if start in seen:
            continue
        loop, prev, cur = [start], start, min(nbr[start])
        seen.add(start)
        while cur != start:
            loop.append(cur)
            seen.add(cur)
            a, b = nbr[cur]
            prev, cur = cur, (b if a == prev else a)
        loops.append(loop)
    return loops


def terminal_of(vertices, loop):
    """(x, y, z, radius): the mean of the loop's vertices weighted by half the sum of their two rim edges, in loop order."""
    p = [np.asarray(vertices, dtype=np.float64).reshape(-1, 3)[i].tolist() for i in loop]
    m = len(p)
    length = [_norm(p[(i + 1) % m][0] - p[i][0], p[(i + 1) % m][1] - p[i][1], p[(i + 1) % m][2] - p[i][2]) for i in range(m)]
    wt = [0.5 * (length[i - 1] + length[i]) for i in range(m)]
    W, S = 0.0, [0.0, 0.0, 0.0]
    for i in range(m):
        W = W + wt[i]
        for c in range(3):
            S[c] = S[c] + wt[i] * p[i][c]
    centre = [S[c] / W for c in range(3)]
    R = 0.0
    for i in range(m):
        R = R + wt[i] * _norm(p[i][0] - centre[0], p[i][1] - centre[1], p[i][2] - centre[2])
    return centre[0], centre[1], centre[2], R / W


def tree(nodes, edges, terminals, min_branch_mm=-1.0):
    """Rule T on node records, node edges and terminals [(x, y, z, radius, node)]: dict(points [(x, y, z, radius, branch,
    node)], branches [(parent_branch, parent_index, ends_in_terminal, n_points)], report)."""
    k, t = len(nodes), len(terminals)
    band = [int(b) for b in nodes["band"]]
    flags = [int(b) for b in nodes["flags"]]
    adj = [[] for _ in range(k)]
    for a, b in np.asarray(edges, dtype=np.int64).reshape(-1, 2).tolist():
        adj[a].append(b)
        adj[b].append(a)
    parent = [-1] * (k + t)
    for n in range(k):
        if not flags[n] & 4:
            lower = [a for a in adj[n] if band[a] < band[n]]
            parent[n] = min(lower) if lower else -1
    # components
    label = list(range(k))
    changed = True
    while changed:
        changed = False
        for n in range(k):
            for a in adj[n]:
                if label[a] < label[n]:
                    label[n] = label[a]
                    changed = True
    components = len(set(label))
    children = [[] for _ in range(k + t)]
    for n in range(k):
        if parent[n] >= 0:
            children[parent[n]].append(n)

    def all_open(n):
        return bool(flags[n] & 1) and all(all_open(c) for c in children[n])

    keep = [parent[n] < 0 or not all_open(n) for n in range(k)] + [True] * t
    pos = [[float(nodes["x"][n]), float(nodes["y"][n]), float(nodes["z"][n])] for n in range(k)]
    rad = [float(nodes["radius"][n]) for n in range(k)]
    for j, (x, y, z, r, node) in enumerate(terminals):
        a = int(node)
        while not keep[a]:
            a = parent[a]
        parent[k + j] = a
        pos.append([float(x), float(y), float(z)])
        rad.append(float(r))
    kids = [[] for _ in range(k + t)]
    for i in range(k + t):
        if keep[i] and parent[i] >= 0:
            kids[parent[i]].append(i)

    def step(a, b):
        return _norm(pos[b][0] - pos[a][0], pos[b][1] - pos[a][1], pos[b][2] - pos[a][2])

    def chain(leaf, stop):
        """leaf's ancestors up to (not including) the first for which stop holds, top first; and that ancestor."""
        out, i = [], leaf
        while i >= 0 and not stop(i):
            out.append(i)
            i = parent[i]
        return out[::-1], i

    def length(top, nodes_down):
        s, a = 0.0, top
        for b in nodes_down:
            s = s + step(a, b)
            a = b
        return s

    points, branches, at, branch_of, pruned = [], [], {}, {}, 0

    def emit(path, junction):
        b = len(branches)
        for i in path:
            at[i] = len(points)
            branch_of[i] = b
            points.append((pos[i][0], pos[i][1], pos[i][2], rad[i], b, i))
        branches.append((branch_of[junction] if junction >= 0 else -1, at[junction] if junction >= 0 else -1,
                         int(path[-1] >= k), len(path)))

    roots = [n for n in range(k) if keep[n] and parent[n] < 0]
    for root in roots:
        def under(i):
            while parent[i] >= 0:
                i = parent[i]
            return i == root
        leaves = [i for i in range(k + t) if keep[i] and not kids[i] and under(i)]
        best, best_len = None, None
        for l in leaves:
            path, _ = chain(l, lambda i: False)
            d = length(path[0], path[1:])
            if best is None or d > best_len:
                best, best_len = path, d
        emit(best, -1)
        free = [l for l in leaves if l not in at]
        while free:
            pick = None
            for l in free:
                path, j = chain(l, lambda i: i in at)
                d = length(j, path)
                if pick is None or d > pick[0]:
                    pick = (d, l, path, j)
            d, l, path, j = pick
            free.remove(l)
            threshold = float(min_branch_mm) if min_branch_mm >= 0 else 2.0 * rad[j]
            if l < k and d < threshold:
                pruned += 1
                continue
            emit(path, j)
    report = {"n_points": len(points), "n_branches": len(branches), "n_roots": len(roots), "n_components": components,
              "n_loops": len(np.asarray(edges).reshape(-1, 2)) - k + components, "n_dropped_open": keep[:k].count(False),
              "n_pruned": pruned, "n_terminals": t}
    return {"points": points, "branches": branches, "report": report}


def tangents(points):
    """recompute_tangents' rule: normalised forward differences inside a branch, the last point repeats, a lone point 0."""
    n = len(points)
    out = []
    for i in range(n):
        if i + 1 < n and points[i][4] == points[i + 1][4]:
            d = [points[i + 1][c] - points[i][c] for c in range(3)]
            nn = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            with np.errstate(all="ignore"):
                out.append([float(np.float64(x) / np.float64(nn)) for x in d])
        elif i > 0 and points[i - 1][4] == points[i][4]:
            out.append(list(out[-1]))
        else:
            out.append([0.0, 0.0, 0.0])
    return out


def centerline(vertices, faces, seeds, h=None, min_branch_mm=-1.0):
    """The composite on the checker: skeleton, the terminals of the rim loops without a seed, the tree."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    h = default_band(v, faces) if h is None else h
    sk = skeleton(v, faces, seeds, h)
    seed_set = set(int(s) for s in seeds)
    terminals = []
    for loop in rim_loops(v.shape[0], faces):
        if seed_set.intersection(loop):
            continue
        terminals.append(terminal_of(v, loop) + (int(sk["vertex_node"][loop[0]]),))
    return dict(tree(sk["nodes"], sk["edges"], terminals, min_branch_mm), skeleton=sk, terminals=terminals)
