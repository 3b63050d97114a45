"""Worst cases for the geodesic field and the band skeleton (include/mm_centerline.h, rules G and S;
csrc/mm_geodesic_kernels.hip, csrc/mm_geodesic.cpp), shared by tests/test_geo_attack_host.py and
tests/test_gpu_geo_attack.py.  Data only: no device and no checker; every case is seeded and built once.

A case is (name, vertices, faces, seeds[, band]).  The kernel relaxes blocks of BLOCK = 256 consecutive vertices, keeps the
first ROW = 8 entries of a vertex's ascending row in registers and walks the rest from memory; the families, by prefix:

* hub_      A closed fan of d spokes round one hub in a mesh of 600 vertices (three blocks, the last one partial).  The
            ring's indices are spread evenly over [0, 600), so the hub's row of length d crosses every block; the rest of
            the vertices are a zigzag strip that carries the field to one ring vertex, the entry.  The ring is laid out
            as a star polygon {d / m}, m about d / 3, with radii jittered in [1, 1.25]: consecutive ring vertices are
            about 120 degrees apart, so only the entry's two ring neighbours take their value along a ring edge and every
            other ring vertex takes it through the hub (two ring edges are longer than two spokes).  On a flat circle
            the front would walk round the ring and every block would run again anyway, which hides a hub that failed to
            flag.  hub_<kind>_<d>_<hub index>: the entry is the hub's predecessor, at rank >= 8 of the hub's row in
            another block (late_out) or in the hub's block (late_in), or at rank < 8 in another block (early_out).
            hub_seed_<d>: the hub is the seed.  hub_meet_<d>: two seeds at the ends of two strips of equal shape.  Strip A
            lies in index order (a few rounds) and enters at a; strip B's indices are shuffled over the other blocks (a
            round a hop) and it enters at b, whose spoke is 0.01 shorter: the hub falls a second time, by 0.01, long after
            everything settled, and every ring vertex but a, b and their ring neighbours must fall with it.  The ring's
            order is a's three, then all ring vertices of the block X that holds none of the hub's first eight entries,
            then b's three, then the rest: no vertex of X has a ring neighbour that falls, strip A holds X's other
            vertices, and so X runs again only if the hub itself flags it.
* detour_   A zigzag chain of unit steps along x (edges of one and of two units), two-hop arches over every eight units (1.2
            a unit) and two-hop spokes from the seed to every sixteenth chain vertex (1.5 a unit): the fewer hops a path
            has, the more it costs, so a vertex takes an early, large value from a spoke and falls again and again as the
            arches and then the chain arrive.  No edge joins the seed and the chain: a spoke and an arch are two faces
            (i, a, b), (a, b, j).  With 20, 30 and 50 spokes (442, 662 and 1102 vertices: 2, 3 and 5 blocks) under a seeded
            permutation of the indices, which parts most neighbours into different blocks, and once in index order.
* weights_  A jittered grid (625 vertices) and strip (600): every vertex scaled by its own 2^k, k in [-30, 30]; the mesh at
            2^-520 (squares partly subnormal), at 2^-600 (every weight +0.0; indices permuted) and at 2^500; a grid at 2^511 with five
            vertices lifted by 1.6 (their two diagonals overflow, they stay connected) and three by 2 (all six edges
            overflow, they are cut off); duplicate points across blocks; a NaN and an inf vertex with neighbours in other
            blocks; overflow_sum, the strip at 1.3 * 2^511, the largest weights the rule can produce -- a finite weight is
            the square root of a finite double and so below 2^512, and fewer than 2^31 of them cannot sum to +inf: the
            case pins that every connected vertex is reached (a path sum that overflows cannot be built from a mesh).
* bands_    With a band.  Strips whose weights are 1, 0.75 and 1.25, so every distance is a multiple of 1 / 4 and
            dist / band is exact for band in {0.5, 1, 3}: the bottom row sits on the band boundaries.  BANDS_EXPECT holds
            (n_nodes, n_node_edges): 1, 2, 3, 4, 5, 255, 256, 257, 4096, 4097 nodes; 256, 257, 4095 and 4096 node edges.
            One non-dyadic band (0.1); a hub mesh in one node (one lane walks every corner and vertex); two fat nodes
            joined by 599 edges of the graph; a permuted strip of 2048 vertices in one band; a strip of four blocks with a
            NaN vertex (non-finite areas) and two pendant vertices behind zero-area faces, all beyond block 0.
"""
import functools
import math

import numpy as np

BLOCK, ROW = 256, 8
NV_HUB = 600


def block_of(i):
    return int(i) // BLOCK


# ---- hubs -----------------------------------------------------------------------------------------------------------------

def star_step(d):
    """The m nearest d / 3 (upwards first) that is coprime to d: the star polygon {d / m} visits every vertex."""
    m = max(2, round(d / 3))
    while math.gcd(m, d) != 1:
        m += 1
    return m


def hub_ring(d, hub):
    """The d ring indices, ascending, spread evenly over the indices other than the hub."""
    others = [i for i in range(NV_HUB) if i != hub]
    return [others[(k * len(others)) // d] for k in range(d)]


def _zigzag(at, direction, m):
    """m points leaving `at` along `direction` in unit steps, every other one 0.3 to the side and all a little up."""
    side = np.array([-direction[1], direction[0], 0.0])
    return [at + direction * (j + 1.0) + side * (0.3 * (j % 2)) + [0.0, 0.0, 0.05 * (j % 3)] for j in range(m)]


def hub_mesh(d, hub, sequence, entries, radius_of=None):
    """The fan and its strips.  sequence[p] = the rank (in the hub's row) of the ring vertex at position p of the star;
    entries = [(ranks, strip indices from the ring outwards)]: a strip that enters at one rank leaves that ring vertex
    outwards, one that enters at two starts half a unit above the hub and climbs; radius_of = {rank: radius} replaces the
    jittered radii.  Returns (vertices, faces, ring, the last vertex of every strip)."""
    ring = hub_ring(d, hub)
    rng = np.random.default_rng(1000 * d + hub)
    m = star_step(d)
    v = np.zeros((NV_HUB, 3))
    radius = 1.0 + 0.25 * rng.random(d)
    theta = 2.0 * math.pi * m * np.arange(d) / d
    for p, rank in enumerate(sequence):
        r = radius[p] if radius_of is None or rank not in radius_of else radius_of[rank]
        v[ring[rank]] = r * np.array([math.cos(theta[p]), math.sin(theta[p]), 0.0])
    f = [[hub, ring[sequence[p]], ring[sequence[(p + 1) % d]]] for p in range(d)]
    ends = []
    for ranks, idx in entries:
        if len(ranks) == 1:
            at = v[ring[ranks[0]]]
            pts = _zigzag(at, at / np.linalg.norm(at), len(idx))
        else:
            pts = [np.array([0.3 * (j % 2), 0.05 * (j % 3), 0.5 + j]) for j in range(len(idx))]
        for i, q in zip(idx, pts):
            v[i] = q
        f += [[ring[r], idx[0], idx[1]] for r in ranks]
        f += [[idx[j], idx[j + 1], idx[j + 2]] for j in range(len(idx) - 2)]
        ends.append(int(idx[-1]))
    return v, np.array(f, dtype=np.int64), ring, ends


def _arrivals(v, f, seed):
    """Plain f64 Dijkstra over the faces' edges, to place a vertex: the distance of every vertex from seed."""
    import heapq
    rows = {}
    for a, b, c in f.tolist():
        for p, q in ((a, b), (b, c), (c, a)):
            w = float(np.linalg.norm(v[p] - v[q]))
            rows.setdefault(p, []).append((q, w))
            rows.setdefault(q, []).append((p, w))
    dist, heap = {seed: 0.0}, [(0.0, seed)]
    while heap:
        x, i = heapq.heappop(heap)
        if x > dist[i]:
            continue
        for j, w in rows[i]:
            if x + w < dist.get(j, math.inf):
                dist[j] = x + w
                heapq.heappush(heap, (x + w, j))
    return dist


def hub_entry_rank(d, hub, kind):
    """A rank of the hub's row of the kind asked for: the middle one of those there are."""
    ring = hub_ring(d, hub)
    late = kind.startswith("late")
    inside = kind.endswith("in")
    ranks = [r for r in range(d) if (r >= ROW) == late and (block_of(ring[r]) == block_of(hub)) == inside]
    if not ranks:
        raise ValueError(f"no {kind} entry for d = {d}, hub = {hub}")
    return ranks[len(ranks) // 2]


def hub_case(d, hub, kind):
    """One seed at the end of one strip that enters at the rank hub_entry_rank gives; kind "seed": the hub is the seed."""
    ring = hub_ring(d, hub)
    rank = 0 if kind == "seed" else hub_entry_rank(d, hub, kind)
    free = [i for i in range(NV_HUB) if i != hub and i not in set(ring)]
    v, f, ring, ends = hub_mesh(d, hub, list(range(d)), [([rank], free[::-1])])
    return v, f, [hub] if kind == "seed" else ends


def hub_meet_plan(d, hub):
    """(X, sequence, (a1, a2), b): the starved block, the ring's order, the ranks where strip A and strip B enter."""
    ring = hub_ring(d, hub)
    fed = {block_of(hub)} | {block_of(ring[r]) for r in range(min(ROW, d))}
    starved = sorted({block_of(i) for i in ring[ROW:]} - fed)
    if not starved:
        raise ValueError(f"the hub's first entries reach every block for d = {d}, hub = {hub}")
    x = starved[0]
    pool = [r for r in range(d) if block_of(ring[r]) != x]
    arc = [r for r in range(d) if block_of(ring[r]) == x]
    assert len(pool) >= 9
    return x, pool[0:3] + arc + pool[3:9] + pool[9:], (pool[1], pool[4]), pool[7]


def hub_meet_case(d, hub):
    ring = hub_ring(d, hub)
    x, sequence, (a1, a2), b = hub_meet_plan(d, hub)
    free = [i for i in range(NV_HUB) if i != hub and i not in set(ring)]
    in_x = [i for i in free if block_of(i) == x]
    rest = [i for i in free if block_of(i) != x]
    m = len(free) // 2
    assert len(in_x) <= m
    take = m - len(in_x)
    strip_a = in_x + rest[:take]                                          # ascending from the ring outwards
    others = rest[take:]
    strip_b = [int(i) for i in np.random.default_rng(d).permutation(others[:m])]
    seed_a, seed_b = strip_a[-1], strip_b[-1]
    strip_a = strip_a + others[m:]                                        # an odd vertex out goes beyond A's seed
    radius_of = {a1: 1.1, a2: 1.101, b: 1.0}
    v, f, _, _ = hub_mesh(d, hub, sequence, [([a1, a2], strip_a), ([b], strip_b)], radius_of)
    # B's strip moves with b, so b's arrival from B does not depend on b's radius: the hub's from B = that + the radius
    radius_of[b] = _arrivals(v, f, seed_a)[hub] - 0.01 - _arrivals(v, f, seed_b)[ring[b]]
    assert 0.5 < radius_of[b] < 2.0
    v, f, _, _ = hub_mesh(d, hub, sequence, [([a1, a2], strip_a), ([b], strip_b)], radius_of)
    return v, f, [seed_a, seed_b]


HUB_SINGLE = [(7, 0, "early_out"), (8, 255, "early_out"), (9, 256, "early_out"), (16, 599, "early_out"), (17, 599, "early_out"),
              (64, 256, "early_out"), (300, 256, "early_out"),
              (9, 0, "late_out"), (16, 255, "late_out"), (17, 256, "late_out"), (64, 0, "late_out"), (300, 599, "late_out"),
              (9, 599, "late_in"), (16, 256, "late_in"), (17, 599, "late_in"), (64, 255, "late_in"), (300, 0, "late_in")]
HUB_SEED = [(8, 599), (9, 0), (64, 256), (300, 255)]
HUB_MEET = [(17, 0), (64, 599), (300, 599)]


def hub_of(name):
    """(d, hub index, kind) of a hub_ case by its name."""
    for d, hub, kind in HUB_SINGLE:
        if name == f"hub_{kind}_{d}_{hub}":
            return d, hub, kind
    for d, hub in HUB_SEED:
        if name == f"hub_seed_{d}":
            return d, hub, "seed"
    for d, hub in HUB_MEET:
        if name == f"hub_meet_{d}":
            return d, hub, "meet"
    raise KeyError(name)


# ---- detours --------------------------------------------------------------------------------------------------------------

def _bridge(v, f, i, j, lift, new):
    """Two faces (i, a, b), (a, b, j): a and b over the middle of i j, `lift` up; they take the indices new, new + 1."""
    mid = 0.5 * (v[i] + v[j])
    v[new] = mid + [0.0, 0.1, lift]
    v[new + 1] = mid + [0.0, -0.1, 1.01 * lift]
    f += [[i, new, new + 1], [new, new + 1, j]]


def detour(n_spokes, permute_seed=None):
    """(vertices, faces, the seed).  The chain c_i = (i, 0.3 (i odd), 0), i <= 16 n_spokes, as a triangle strip; the seed at
    (-1, 0, 0); a spoke to every c_16k lifted by 0.559 of its length (1.5 a unit), an arch over every c_8j c_8j+8 lifted
    by 2.65 (1.2 a unit)."""
    n = 16 * n_spokes + 1
    nv = n + 1 + 2 * n_spokes + 4 * n_spokes
    v = np.zeros((nv, 3))
    v[:n, 0] = np.arange(n)
    v[:n, 1] = 0.3 * (np.arange(n) % 2)
    seed = n
    v[seed] = [-1.0, 0.0, 0.0]
    f = [[i, i + 1, i + 2] for i in range(n - 2)]
    new = n + 1
    for k in range(n_spokes):
        _bridge(v, f, seed, 16 * k, 0.559 * float(np.linalg.norm(v[16 * k] - v[seed])), new)
        new += 2
    for j in range(2 * n_spokes):
        _bridge(v, f, 8 * j, 8 * j + 8, 2.65, new)
        new += 2
    assert new == nv
    f = np.array(f, dtype=np.int64)
    if permute_seed is None:
        return v, f, seed
    p = np.random.default_rng(permute_seed).permutation(nv)              # old index -> new index
    out = np.empty_like(v)
    out[p] = v
    return out, p[f], int(p[seed])


# ---- weights --------------------------------------------------------------------------------------------------------------

def grid(n=24):
    """n x n unit squares cut along one diagonal; vertex (row i, column j) has index i (n + 1) + j."""
    j, i = np.meshgrid(np.arange(n + 1), np.arange(n + 1))
    v = np.stack([i.ravel().astype(float), j.ravel().astype(float), np.zeros((n + 1) ** 2)], 1)
    q = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
    f = np.concatenate([np.stack([q, q + 1, q + n + 2], 1), np.stack([q, q + n + 2, q + n + 1], 1)]).astype(np.int64)
    return v, f


def strip(n, rise=1.0, shift=0.25, permute_seed=None):
    """2 x n vertices, bottom i at (i, 0, 0), top n + i at (i + shift, rise, 0); faces (i, i + 1, n + i), (i + 1, n + i + 1,
    n + i).  With rise = 0.75 and shift = 0 the weights are 1, 0.75 and 1.25.  Returns (vertices, faces, the index of
    bottom 0)."""
    x = np.arange(n, dtype=np.float64)
    v = np.concatenate([np.stack([x, np.zeros(n), np.zeros(n)], 1), np.stack([x + shift, np.full(n, rise), np.zeros(n)], 1)])
    i = np.arange(n - 1)
    f = np.concatenate([np.stack([i, i + 1, n + i], 1), np.stack([i + 1, n + i + 1, n + i], 1)]).astype(np.int64).reshape(-1, 3)
    if permute_seed is None:
        return v, f, 0
    p = np.random.default_rng(permute_seed).permutation(2 * n)
    out = np.empty_like(v)
    out[p] = v
    return out, p[f], int(p[0])


def _jittered(v, seed):
    return v + np.random.default_rng(seed).uniform(-0.2, 0.2, v.shape)


LIFTED_PARTLY = [(2, 2), (2, 6), (10, 10), (20, 5), (12, 20)]            # grid (row, column): the two diagonals overflow
LIFTED_OFF = [(5, 5), (15, 15), (11, 3)]                                 # all six edges overflow
NAN_VERTEX, INF_VERTEX = 260, 510                                        # grid (10, 10) and (20, 10): neighbours 235 and 535
DUPLICATES = [(250, 275), (505, 530), (10, 600)]                         # the first two are neighbours across a block border


def _weights_cases():
    gv, gf = grid(24)
    sv, sf, _ = strip(300)
    gj, sj = _jittered(gv, 31), _jittered(sv, 32)
    out = []
    for tag, v, f in (("grid", gj, gf), ("strip", sj, sf)):
        k = np.random.default_rng(33).integers(-30, 31, len(v))
        out.append((f"weights_scales_{tag}", v * (2.0 ** k)[:, None], f, [0]))
        out.append((f"weights_2m520_{tag}", v * 2.0 ** -520, f, [0]))
        p = np.random.default_rng(34).permutation(len(v))                # old index -> new: local index minima all over
        pv = np.empty_like(v)
        pv[p] = v
        out.append((f"weights_2m600_{tag}", pv * 2.0 ** -600, p[f], [int(p[0])]))
        out.append((f"weights_2p500_{tag}", v * 2.0 ** 500, f, [0]))
    v = gv.copy()
    for (r, c) in LIFTED_PARTLY:
        v[r * 25 + c, 2] = 1.6
    for (r, c) in LIFTED_OFF:
        v[r * 25 + c, 2] = 2.0
    out.append(("weights_overflow_some_grid", v * 2.0 ** 511, gf, [0]))
    out.append(("weights_overflow_sum_strip", sv * (1.3 * 2.0 ** 511), sf, [0]))
    v = gj.copy()
    for a, b in DUPLICATES:
        v[b] = v[a]
    out.append(("weights_duplicates_grid", v, gf, [0]))
    v = gj.copy()
    v[NAN_VERTEX] = np.nan
    v[INF_VERTEX, 0] = np.inf
    out.append(("weights_nan_inf_grid", v, gf, [0]))
    return out


# ---- bands ----------------------------------------------------------------------------------------------------------------

BANDS_EXPECT = {}                                                        # name: (n_nodes, n_node_edges)
PLAIN_N, PLAIN_NAN, PLAIN_PENDANTS = 400, 300, (350, 390)                # the strip, the top vertex that is NaN, the pendants' feet


def _bands_cases():
    out = []

    def dyadic(n):
        v, f, _ = strip(n, rise=0.75, shift=0.0)
        return v, f

    # seeded at bottom 0: bottom i is at i, top i at i + 0.75.  band 1: {bottom i, top i} is node i, n nodes, n - 1 edges
    v, f = dyadic(2)
    out.append(("bands_nodes_1", v, f, [0], 3.0))
    BANDS_EXPECT["bands_nodes_1"] = (1, 0)
    for n in (2, 3, 4, 5, 255, 256, 257, 4096, 4097):
        v, f = dyadic(n)
        out.append((f"bands_nodes_{n}", v, f, [0], 1.0))
        BANDS_EXPECT[f"bands_nodes_{n}"] = (n, n - 1)
    # band 0.5: bottom i is band 2 i, top i band 2 i + 1, every vertex a node; 3 (n - 1) + n edges
    v, f = dyadic(65)
    out.append(("bands_half_65", v, f, [0], 0.5))
    BANDS_EXPECT["bands_half_65"] = (130, 257)
    # band 3: bottom and top i in band i // 3
    v, f = dyadic(768)
    out.append(("bands_three_768", v, f, [0], 3.0))
    BANDS_EXPECT["bands_three_768"] = (256, 255)
    v, f = dyadic(30)
    out.append(("bands_tenth_30", v, f, [0], 0.1))                       # counts left to the oracle: 0.1 is no dyadic number
    d, hub, kind = HUB_SINGLE[11]
    hv, hf, hs = hub_case(d, hub, kind)
    out.append(("bands_hub_one_node", hv, hf, hs, 1.0e6))
    BANDS_EXPECT["bands_hub_one_node"] = (1, 0)
    v, f = dyadic(300)
    out.append(("bands_two_fat", v, f, list(range(300)), 0.5))           # the bottom row at 0, the top row at 0.75
    BANDS_EXPECT["bands_two_fat"] = (2, 1)
    v, f, s = strip(1024, permute_seed=41)
    out.append(("bands_one_band_permuted", v, f, [s], 1.0e6))
    BANDS_EXPECT["bands_one_band_permuted"] = (1, 0)
    v, f = dyadic(PLAIN_N)
    v[PLAIN_N + PLAIN_NAN] = np.nan
    extra, faces = [], []
    for k, foot in enumerate(PLAIN_PENDANTS):                            # a vertex 1.5 below, behind the face (foot, p, p)
        p = 2 * PLAIN_N + k
        extra.append(v[foot] + [0.0, -1.5, 0.0])
        faces.append([foot, p, p])
    out.append(("bands_plain_mean", np.concatenate([v, extra]), np.concatenate([f, np.array(faces, dtype=np.int64)]), [0], 1.0))
    BANDS_EXPECT["bands_plain_mean"] = (PLAIN_N + 2, PLAIN_N - 1 + 2)
    return out


# ---- all of them ------------------------------------------------------------------------------------------------------------

DETOURS = [("detour_2_blocks", 20, 51), ("detour_3_blocks", 30, 52), ("detour_5_blocks", 50, 53), ("detour_in_order", 30, None)]


@functools.lru_cache(maxsize=None)
def cases():
    """{name: (name, vertices f64[nv, 3], faces int64[nf, 3], seeds int64[n][, band])}, built once."""
    out = []
    for d, hub, kind in HUB_SINGLE:
        out.append((f"hub_{kind}_{d}_{hub}",) + hub_case(d, hub, kind))
    for d, hub in HUB_SEED:
        out.append((f"hub_seed_{d}",) + hub_case(d, hub, "seed"))
    for d, hub in HUB_MEET:
        out.append((f"hub_meet_{d}",) + hub_meet_case(d, hub))
    for name, n_spokes, permute_seed in DETOURS:
        v, f, s = detour(n_spokes, permute_seed)
        out.append((name, v, f, [s]))
    out += _weights_cases()
    out += _bands_cases()
    done = {}
    for c in out:
        v = np.ascontiguousarray(c[1], dtype=np.float64)
        f = np.ascontiguousarray(c[2], dtype=np.int64).reshape(-1, 3)
        v.setflags(write=False)
        f.setflags(write=False)
        assert c[0] not in done and len(v) <= (9000 if c[0].startswith("bands_") else 1500)
        done[c[0]] = (c[0], v, f, np.array(c[3], dtype=np.int64)) + tuple(c[4:])
    return done


def family(name):
    return name.split("_")[0]


NAMES = tuple(cases())
FIELD_NAMES = tuple(n for n in NAMES if family(n) != "bands")
BANDS_NAMES = tuple(n for n in NAMES if family(n) == "bands")
