"""Worst cases for the mesh relaxation (include/mm_ccta.h, "mesh relaxation"; csrc/mm_relax_kernels.hip, the seeded search
of csrc/mm_tri_kernels.hip), shared by tests/test_relax_attack_host.py and tests/test_gpu_relax_attack.py.  Data only:
no device and no checker of the relaxation; every case is seeded and built once.

A case is (name, mesh, reference or None, pinned or None, iterations, lambda).  The families, by the name's prefix:

* ties_     A planar reference of dyadic coordinates, every tooth of a saw present twice.  Every face has one corner at
            x = 0 and two at x = 1, so all slab keys are equal, the plan keeps the index order (mm_prune.h: sc = 0) and
            a face and its copy, 294 indices apart, lie in different chunks (0 | 1 and 1 | 2).  Six teeth have no copy.
            The mesh: two small grids floating over the saw, one across the teeth without a copy.  "shuffled": the same
            faces in a seeded random order.  "filled": the triangles between the teeth too, so the keys differ, the plan
            sorts, and a copy follows its face at once in the staged order but for the chunk borders that part them.
* stale_    A long tube (3 chunks along its axis) and a ring of 513 free vertices around it whose only other neighbours
            are two rims near the far end: long skinny faces.  One step at lambda = 1 carries both query blocks 14 units
            up the tube, from the middle chunk into the last one; lambda = -1 flings them down into the first, and then
            past the tube's end.
* wide_     The same tube; a ring of 512 free vertices between two rims half a unit away, and one free vertex R of it put
            0.4 above the ring.  R's neighbours in the ring are pinned, so no free vertex has R for a neighbour: lambda =
            8 and 64 throw R alone, 2.8 and 25.2 units, and the block's box then covers the tube.  ROGUE[name] = R.
* offset_ / scale_   A jittered tube of 257 free vertices on the unjittered one (510 faces, two chunks), translated by
            2^20 and 2^36 times (1, -3/4, 1/2), scaled by 2^-200, 2^200 and 2^600 (every d2 overflows: nothing moves).
* seed_     The previous face is degenerate (a repeated index, a zero cross product), thin or just not thin (the needle,
            cap and collinear families of tests/tri_sliver_cases.py), or gives a NaN: a face of edge 2^400 whose corner
            wins step 0 and whose interior formula overflows to inf - inf for the candidate.  The meshes are clouds of
            small tetrahedra, one corner at a query of the family.
* grid_     A planar "union-jack" grid (interior valences 4 and 8, so 1 / deg is exact) of dyadic coordinates that is
            its own reference; lambda in {0.5, 1, 2, -1, 4}.  Everything up to the projection is exact in f64.
"""
import functools

import numpy as np

import tri_sliver_cases as SL

CHUNK, QPB = 256, 512


def tube(n_around, n_rings, dz=1.0):
    """A closed tube of radius 1 along z, one winding all over (outward): the wall ring by ring, then the two caps."""
    a = 2.0 * np.pi * np.arange(n_around) / n_around
    ring = np.column_stack([np.cos(a), np.sin(a), np.zeros(n_around)])
    v = np.concatenate([ring + [0.0, 0.0, r * dz] for r in range(n_rings)] + [[[0.0, 0.0, 0.0], [0.0, 0.0, (n_rings - 1) * dz]]])
    f = []
    for r in range(n_rings - 1):
        for k in range(n_around):
            i, j = r * n_around + k, r * n_around + (k + 1) % n_around
            f += [[i, j, j + n_around], [i, j + n_around, i + n_around]]
    c0, top = n_rings * n_around, (n_rings - 1) * n_around
    f += [[c0, (k + 1) % n_around, k] for k in range(n_around)]
    f += [[c0 + 1, top + k, top + (k + 1) % n_around] for k in range(n_around)]
    return v, np.array(f, dtype=np.int64)


def rings_mesh(zs, n):
    """Rings of n vertices at radius 1 and heights zs, joined ring to ring (outward winding, zs ascending)."""
    a = 2.0 * np.pi * np.arange(n) / n
    v = np.concatenate([np.column_stack([np.cos(a), np.sin(a), np.full(n, z)]) for z in zs])
    f = []
    for r in range(len(zs) - 1):
        for k in range(n):
            i, j = r * n + k, r * n + (k + 1) % n
            f += [[i, j, j + n], [i, j + n, i + n]]
    return v, np.array(f, dtype=np.int64)


# ---- ties across chunks --------------------------------------------------------------------------------------------------

TEETH, LONE = 288, 6            # teeth with a copy, teeth without
W = 2.0 ** -9                   # a tooth's width along y


def saw(shuffled=False):
    """(vertices, faces): tooth j = apex (0, (j + 1/2) W), base (1, j W) - (1, (j + 1) W); the faces 0 .. 287 and their
    copies 294 .. 581, the lone teeth 288 .. 293 between them."""
    t = TEETH + LONE
    apex = np.column_stack([np.zeros(t), (np.arange(t) + 0.5) * W, np.zeros(t)])
    base = np.column_stack([np.ones(t + 1), np.arange(t + 1) * W, np.zeros(t + 1)])
    one = np.array([[j, t + j, t + j + 1] for j in range(t)], dtype=np.int64)
    f = np.concatenate([one, one[:TEETH]])
    if shuffled:
        f = f[np.random.default_rng(77).permutation(len(f))]
    return np.concatenate([apex, base]), f


FILLED = 150                    # teeth of the filled saw


def saw_filled():
    """(vertices, faces): 150 teeth and the 149 triangles between them (apex j, base j + 1, apex j + 1: two corners at
    x = 0), tooth and gap in turn, then the 299 copies in the same order.  The slab keys are 2 and 1, so the plan sorts:
    gaps, their copies, teeth, their copies -- and chunk borders fall inside the copies (at staged 256) and inside the
    teeth (at 512)."""
    t = FILLED
    apex = np.column_stack([np.zeros(t), (np.arange(t) + 0.5) * W, np.zeros(t)])
    base = np.column_stack([np.ones(t + 1), np.arange(t + 1) * W, np.zeros(t + 1)])
    one = []
    for j in range(t):
        one.append([j, t + j, t + j + 1])
        if j + 1 < t:
            one.append([j, t + j + 1, j + 1])
    one = np.array(one, dtype=np.int64)
    return np.concatenate([apex, base]), np.concatenate([one, one])


def floating_grids(firsts=(100, 279), shift=0.0):
    """Two grids of 5 x 32 vertices at z = 1/4: x = 1/2 .. 3/4, y every W / 2 from tooth 100 and from tooth 279 (the
    second ends over the lone teeth), every y moved by +- W / 8 -- never on the line between two teeth, where two
    different faces tie, and for the free vertices (x = 9/16 .. 11/16) never over an edge of a tooth.  shift: W / 4 for
    the filled saw, where evenly spaced rows would otherwise settle on the middles of teeth and gaps."""
    rng = np.random.default_rng(5)
    vs, fs = [], []
    for first in firsts:
        base = len(vs)
        sign = rng.integers(0, 2, (5, 32)) * 2 - 1
        for i in range(5):
            for j in range(32):
                vs.append([0.5 + i / 16.0, first * W + j * W / 2.0 + shift + sign[i, j] * W / 8.0, 0.25])
        for i in range(4):
            for j in range(31):
                a = base + i * 32 + j
                fs += [[a, a + 32, a + 33], [a, a + 33, a + 1]]
    return np.array(vs), np.array(fs, dtype=np.int64)


# ---- stale bounds and the wide block -------------------------------------------------------------------------------------

def long_reference():
    return tube(8, 41)          # 656 faces: three chunks along z


def flung_ring():
    """513 free vertices at z = 18.5 between rims at z = 39 and 39.5 (border vertices: they keep their bits)."""
    v, f = rings_mesh([18.5, 39.0], 513)
    n = 513
    top = np.column_stack([v[:n, 0], v[:n, 1], np.full(n, 39.5)])
    v = np.concatenate([v, top])
    # the second band hangs the ring below the upper rim as well: ring -> upper rim, wound the other way round so that
    # every ring edge has its two owners traversing it in opposite directions
    g = []
    for k in range(n):
        i, j = k, (k + 1) % n
        g += [[j, i, 2 * n + i], [j, 2 * n + i, 2 * n + j]]
    return v, np.concatenate([f, np.array(g, dtype=np.int64)])


ROGUE = {}


def rogue_ring():
    """(vertices, faces, pinned, R): rims at z = 33.5 and 34.5, a ring of 514 at z = 34 between them, R = its vertex 0 at
    z = 34.4, its ring neighbours 1 and 513 pinned: 512 free vertices, one query block."""
    n = 514
    v, f = rings_mesh([33.5, 34.0, 34.5], n)
    v[n, 2] = 34.4
    pinned = np.zeros(len(v), dtype=bool)
    pinned[[n + 1, n + n - 1]] = True
    return v, f, pinned, n


# ---- offsets and scales ----------------------------------------------------------------------------------------------------

def jittered_on_plain():
    rv, rf = tube(15, 17)
    return (rv + 0.05 * np.random.default_rng(3).standard_normal(rv.shape), rf), (rv, rf)


def moved(shift=0.0, scale=1.0):
    (v, f), (rv, rf) = jittered_on_plain()
    s = shift * np.array([1.0, -0.75, 0.5])
    return ((v + s) * scale, f), ((rv + s) * scale, rf)


# ---- seeds -----------------------------------------------------------------------------------------------------------------

def tetrahedra(points, size):
    """One small tetrahedron a point, the point its corner 0: closed, so all four corners are free."""
    e = size * np.eye(3)
    v = np.concatenate([[p, p + e[0], p + e[1], p + e[2]] for p in points])
    one = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int64)
    return v, np.concatenate([one + 4 * k for k in range(len(points))])


def sliver_cloud(family):
    """The family's faces as the reference; 132 of its queries (every eleventh or so, 528 free vertices: two blocks)."""
    rv, rf, q = SL.families()[family]
    q = q.reshape(-1, 3)
    return tetrahedra(q[::max(1, len(q) // 132)][:132], 2.0 ** -6), (rv, rf)


def floor(z=-3.0):
    """Eight proper faces: a 2 x 2 square grid of side 4 around the z axis, at height z."""
    v = np.array([[x, y, z] for x in (-4.0, 0.0, 4.0) for y in (-4.0, 0.0, 4.0)])
    f = []
    for i in range(2):
        for j in range(2):
            a = 3 * i + j
            f += [[a, a + 3, a + 4], [a, a + 4, a + 1]]
    return v, np.array(f, dtype=np.int64)


def antennas():
    """The floor and, as faces 0 .. 2, an (a, a, b) face, an (a, b, a) face and three collinear corners: segments that
    stand up from it.  A tetrahedron at every quarter of each: their corners land on the segments at step 0."""
    fv, ff = floor(0.0)
    n = len(fv)
    v = np.concatenate([fv, [[1.0, 1.0, 0.0], [1.0, 1.0, 2.0], [-2.0, 1.0, 0.0], [-2.0, 1.0, 2.0], [1.0, -2.0, 0.5],
                             [1.0, -2.0, 1.5], [1.0, -2.0, 2.5]]])
    f = np.concatenate([[[n, n, n + 1], [n + 2, n + 3, n + 2], [n + 4, n + 5, n + 6]], ff])
    pts = [[x + 0.01, y - 0.02, z] for x, y in ((1.0, 1.0), (-2.0, 1.0), (1.0, -2.0)) for z in (0.75, 1.25, 1.75, 2.25)]
    return tetrahedra(np.array(pts), 2.0 ** -5), (v, f)


def nan_seed():
    """Face 0 = (0, 2^400 e1, 2^400 (e1 + e2)): acute at its corner a = 0.  Corner 0 of every tetrahedron lies behind a
    (region 1: the corner wins step 0 with a finite d2) and is free; the three others, pinned, lie inside the wedge a
    few units around it.  The candidate follows their mean: there d5 d2 - d1 d6 is -inf + inf, the interior formula gives
    NaN, and the seed stays at +inf.  The floor at z = -1/2 takes the vertex."""
    fv, ff = floor(-0.5)
    n = len(fv)
    big = 2.0 ** 400
    v = np.concatenate([fv, [[0.0, 0.0, 0.0], [big, 0.0, 0.0], [big, big, 0.0]]])
    f = np.concatenate([[[n, n + 1, n + 2]], ff])
    tv, tf = [], []
    for k in range(6):                                                    # the pinned corners far off: no face turns
        p = np.array([-0.0625 - 0.0078125 * k, -0.125 + 0.00390625 * k, 0.015625 * (k % 3)])
        base = len(tv)
        tv += [p, [8.0, 1.0 + 0.125 * k, 4.0], [8.0, 4.0, -4.0 - 0.25 * k], [-6.0 + 0.25 * k, -2.0, 0.25]]
        tf += [[base, base + 2, base + 1], [base, base + 1, base + 3], [base, base + 3, base + 2],
               [base + 1, base + 2, base + 3]]
    tv = np.array(tv)
    pinned = np.ones(len(tv), dtype=bool)
    pinned[::4] = False
    return (tv, np.array(tf, dtype=np.int64)), (v, f), pinned


# ---- the exact grid ----------------------------------------------------------------------------------------------------------

GRID = 10                       # quads a side


def union_jack():
    """(GRID + 1)^2 vertices at integer (i, j), z = 0; quad (i, j) is cut from (i, j) to (i + 1, j + 1) where i + j is
    even, the other way where it is odd: valence 8 at even interior vertices, 4 at odd ones.  The vertices 2 .. 8 of
    each axis are moved by multiples of 1/16 up to 3/16, so no candidate leaves the grid and no face of the input is
    turned."""
    m = GRID + 1
    rng = np.random.default_rng(19)
    v = np.array([[float(i), float(j), 0.0] for i in range(m) for j in range(m)])
    for i in range(2, m - 2):
        for j in range(2, m - 2):
            v[i * m + j, :2] += rng.integers(-3, 4, 2) / 16.0
    f = []
    for i in range(GRID):
        for j in range(GRID):
            a, b, c, d = i * m + j, (i + 1) * m + j, (i + 1) * m + j + 1, i * m + j + 1
            f += [[a, b, c], [a, c, d]] if (i + j) % 2 == 0 else [[a, b, d], [b, c, d]]
    return v, np.array(f, dtype=np.int64)


GRID_LAMBDAS = (0.5, 1.0, 2.0, -1.0, 4.0)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (name, mesh, reference or None, pinned or None, iterations, lambda)."""
    out = []
    for name, ref, grids in (("ties", saw(), floating_grids()), ("ties_shuffled", saw(True), floating_grids()),
                             ("ties_filled", saw_filled(), floating_grids((100, 130), W / 4.0))):
        for it in (0, 1, 3):
            out.append((f"{name}_{it}", grids, ref, None, it, 1.0))
    ring = flung_ring()
    out.append(("stale_up", ring, long_reference(), None, 1, 1.0))
    out.append(("stale_down_twice", ring, long_reference(), None, 2, -1.0))
    rv, rf, pinned, r = rogue_ring()
    for lamb in (8.0, 64.0):
        out.append((f"wide_{int(lamb)}", (rv, rf), long_reference(), pinned, 1, lamb))
        ROGUE[f"wide_{int(lamb)}"] = r
    for name, shift in (("offset_2p20", 2.0 ** 20), ("offset_2p36", 2.0 ** 36)):
        mesh, ref = moved(shift=shift)
        out.append((name + "_project", mesh, ref, None, 0, 0.5))
        out.append((name, mesh, ref, None, 2, 0.5))
    for name, scale in (("scale_2m200", 2.0 ** -200), ("scale_2p200", 2.0 ** 200), ("scale_2p600", 2.0 ** 600)):
        mesh, ref = moved(scale=scale)
        out.append((name, mesh, ref, None, 2, 0.5))
    for family in ("needle_axis", "cap_random", "collinear"):
        mesh, ref = sliver_cloud(family)
        out.append((f"seed_{family}_project", mesh, ref, None, 0, 0.5))
        out.append((f"seed_{family}", mesh, ref, None, 2, 0.5))
    mesh, ref = antennas()
    out.append(("seed_degenerate", mesh, ref, None, 2, 0.5))
    mesh, ref, pinned = nan_seed()
    out.append(("seed_nan", mesh, ref, pinned, 1, 0.5))
    for lamb in GRID_LAMBDAS:
        out.append((f"grid_{lamb:g}", union_jack(), None, None, 1, lamb))
    return {c[0]: c for c in out}


NAMES = tuple(cases())


def family(name):
    return name.split("_")[0]
