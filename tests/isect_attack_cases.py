"""Worst cases for the soundness promise of the mesh intersection check (include/mm_ccta.h, "mesh intersections"): a pair
reported disjoint or intersecting is so in exact arithmetic, whatever is doubtful is undecided.  Shared by
tests/test_intersect_attack_host.py (the checker and csrc/mm_isect_device.h as a host program, no device) and
tests/test_gpu_intersect_attack.py (the kernel against the checker).  Deterministic: fixed seeds, no device.

A case is (t1, t2, id1, id2, family): two faces as 3-tuples of 3-tuples of floats and the canonical ids of their corners,
which are always those of equal coordinates (X.canonical_ids of the six corners), so a mesh that holds the six corners
as six vertices recreates them.  A pair with a face that is degenerate by the rule (a rounded normal of exactly zero)
is not a case.  The oracle is tests/test_intersect_host.py's, in fractions.Fraction; `meets` remembers its answers by
the coordinates and by which corners are shared, which is all the oracle reads.

Families (`family(name)`; `kinds(name)` says which construction made each case), each about a few random base triangles
with corners in [-2, 2]^3; "stepped" is test_intersect_host._steps: 0, +-1 .. +-6 ulp and +-4 * 2^-k, k = 30 .. 52.
* corner: the constructions of test_every_proved_state_is_true_near_a_plane_and_near_an_edge_line -- one corner of face 2
  stepped off the plane of face 1 (inside it) and off the line of its edge a b, with no, one and two shared vertices, a
  coplanar partner, and coplanar partners at a shared corner in the opposite wedge and beside an edge.
* edge_edge: no shared vertex; the edge p q of face 2 passes through a point of the edge a b of face 1, both in their
  interiors, and p is stepped along the axis of the largest component of (b - a) x (q - p), so the edges pass each other
  on either side: the interval predicates e1, e2 of the Guigue-Devillers test near zero.  The third corner of face 2
  lies on either side of p q, because only one of the two sides lets the faces come apart.  Both orders.
* one_shared_edge: the faces share the corner a.  The opposite edge q r of face 2 passes within steps of the opposite
  edge b c of face 1 ("bc": a common segment from a stays, so never disjoint), of the edge a b at the shared corner
  ("ab": disjoint where it passes outside) and of the shared corner itself ("at_corner": face 2 a needle through a).
  Every step runs under three of the nine pairs of rotations of the two corner orders; all nine occur.
* two_shared: the faces share the edge a b; the unshared corner of face 2 is stepped through the plane of face 1 inside
  face 1 ("folded"), across the shared edge ("flat"), beyond the corner b ("beyond") and 2^-20 beside the line of the
  shared edge on either side ("beside_in", "beside_out").  Every step under three of the eighteen combinations of
  rotations and windings of the shared edge; all eighteen occur.
* sliver: face 1 has its third corner 2^-20, 2^-30, 2^-40, 2^-50 from the middle of its long edge; an edge of the partner
  crosses the sliver's plane at the long edge, offset towards the third corner by 0, +-1e-15, +-1e-13, +-1e-9.  Both
  orders.
* scaled: `subset()`, a fixed choice from the five families above, times 2^k: `scaled(k)`, aligned with `subset()`.
  The subset takes only constructions whose two faces touch or cross within the steps: at the ends of the range every
  orient3d is uncertain and what remains are the 2-D tests, which prove separated projections and nothing else, so a
  pair in contact is undecided there.  The flat pairs, "beside_out", the wedge partners and the needles of "at_corner"
  meet in their shared vertices alone, are separated in 2-D at any scale, and are left out.  After the blocks of
  `scaled(k)` come `guard_cases()`, times a factor that is not a power of two and puts one value within 1e-4 and within
  1e-9 of the 2^-900 guard, on either side: a permanent of every sixteenth case of the subset near 2^-300 (guard_3d), and
  a detsum near 2^-450 of pairs that the 2-D tests prove disjoint -- the constructions the subset leaves out, and pairs
  that lie apart (guard_2d).  Only the lower half of each guard can be observed: a permanent or detsum that overflows
  makes the bound infinite, and no determinant exceeds that, with or without the test against DBL_MAX.
* shifted: the subset translated by 2^20 and by 2^40 along every axis and rounded; ids from the rounded coordinates.
* lattice: the 1 500 integer pairs of test_lattice_pairs_with_exact_contact_are_never_proved_wrong, and one face against
  its six reorderings, which are coincident.
"""
import functools
import itertools

import numpy as np

from mm_checkers import mesh_intersections as X
from test_intersect_host import T, _steps, oracle

D, I, U = X.DISJOINT, X.INTERSECTING, X.UNDECIDED
INF = float("inf")
BUILT = ("corner", "edge_edge", "one_shared_edge", "two_shared", "sliver")      # the constructions; `subset` draws on them
FAMILIES = BUILT + ("scaled", "shifted", "lattice")
SCALES_SAME = (-250, -100, 100, 250)                    # the state must be that of the unscaled case
SCALES_SOUND = (-310, -300, -290, 330, 340, 345)        # the guards bite: soundness only
SCALE_ENDS = (-310, 345)                                # nothing is proved
SHIFTS = (2.0 ** 20, 2.0 ** 40)
SUBSET_PER_FAMILY = 40
OFF_SUBSET = ("wedge", "flat", "beside_out", "at_corner")   # separated in 2-D at any scale
SLIVER_OFFSETS = (0.0, 1e-15, -1e-15, 1e-13, -1e-13, 1e-9, -1e-9)
BATCH_CASES = 256                                       # 512 faces: two chunks of the kernel
BATCH_CASES_OF = {"lattice": 96}                        # every pair of its faces is near and one in four crosses: the oracle's time


def _rot(t, r):
    return (t[r], t[(r + 1) % 3], t[(r + 2) % 3])


def make_case(t1, t2, family, shared=None):
    """The case of two faces, ids by equal coordinates; None where a face is degenerate by the rule."""
    v = np.array(t1 + t2, dtype=np.float64)
    ids = X.canonical_ids(v)
    id1, id2 = tuple(int(x) for x in ids[:3]), tuple(int(x) for x in ids[3:])
    with np.errstate(all="ignore"):
        if X.is_degenerate(v[:3], id1) or X.is_degenerate(v[3:], id2):
            return None
    assert shared is None or n_shared((t1, t2, id1, id2, family)) == shared, (t1, t2, family)
    return (t1, t2, id1, id2, family)


def n_shared(case):
    return sum(i in case[3] for i in case[2])


class _Family:
    def __init__(self, name):
        self.name, self.cases, self.kinds = name, [], []

    def add(self, t1, t2, kind, shared=None):
        c = make_case(t1, t2, self.name, shared)
        if c is not None:
            self.cases.append(c)
            self.kinds.append(kind)


def _moved(base, ax, x):
    p = base.copy()
    p[ax] = x
    return p


def _corner(fam):
    rng = np.random.default_rng(23)
    for trial in range(2):
        a, b, c = rng.uniform(-2.0, 2.0, (3, 3))
        wa, wb = rng.uniform(0.1, 0.45, 2)
        on_plane = a + wa * (b - a) + wb * (c - a)
        on_edge = a + wa * (b - a)
        t1 = T(a, b, c)
        far1, far2 = on_plane + rng.uniform(-1.0, 1.0, 3), on_plane + rng.uniform(-1.0, 1.0, 3)
        ax = int(np.argmax(np.abs(np.cross(b - a, c - a))))
        q1 = a + 0.3 * (b - a) + 1.5 * (c - a)
        q2 = a + 1.5 * (b - a) + 1.6 * (c - a)
        w1, w2 = a - 0.7 * (b - a) - 0.2 * (c - a), a - 0.1 * (b - a) - 0.9 * (c - a)
        for where, base in (("plane", on_plane), ("line", on_edge)):
            for x in _steps(float(base[ax]), 4.0):
                p = _moved(base, ax, x)
                fam.add(t1, T(p, far1, far2), where + "_none", 0)
                fam.add(T(p, far1, far2), t1, where + "_none", 0)
                fam.add(t1, T(a, p, far1), where + "_one", 1)
                fam.add(t1, T(a, far1, p), where + "_one", 1)
                fam.add(t1, T(b, a, p), where + "_two", 2)
                fam.add(t1, T(p, q1, q2), where + "_coplanar", 0)
                for other in (T(a, w1, w2), T(a, p, w2), T(a, w1, p)):
                    fam.add(t1, other, "wedge", 1)


def _edge_edge(fam):
    rng = np.random.default_rng(101)
    for trial in range(3):
        a, b, c = rng.uniform(-2.0, 2.0, (3, 3))
        x = a + rng.uniform(0.3, 0.7) * (b - a)                           # on the edge a b, up to rounding
        d = rng.uniform(-1.0, 1.0, 3)
        s, u = rng.uniform(0.4, 1.0, 2)
        p0, q = x - s * d, x + u * d                                      # the edge of face 2 through x
        off = rng.uniform(-1.0, 1.0, 3)
        ax = int(np.argmax(np.abs(np.cross(b - a, q - p0))))
        t1 = T(a, b, c)
        for side, far in (("near", x + off), ("away", x - off)):
            for val in _steps(float(p0[ax]), 4.0):
                t2 = T(_moved(p0, ax, val), q, far)
                fam.add(t1, t2, side, 0)
                fam.add(t2, t1, side, 0)


def _one_shared_edge(fam):
    rng = np.random.default_rng(103)
    for trial in range(3):
        a, b, c = rng.uniform(-2.0, 2.0, (3, 3))
        t1 = T(a, b, c)
        w = rng.uniform(0.3, 0.7)
        for kind, x, along in (("bc", b + w * (c - b), c - b), ("ab", a + w * (b - a), b - a), ("at_corner", a, b - a)):
            d = rng.uniform(-1.0, 1.0, 3)
            s, u = rng.uniform(0.4, 1.0, 2)
            q0, r = x - s * d, x + u * d
            ax = int(np.argmax(np.abs(np.cross(along, r - q0))))
            for i, val in enumerate(_steps(float(q0[ax]), 4.0)):
                t2 = T(a, _moved(q0, ax, val), r)
                for j in range(3):
                    fam.add(_rot(t1, j), _rot(t2, (i + j) % 3), kind, 1)


TWO_SHARED_COMBOS = tuple((r1, r2, wind) for wind in range(2) for r1 in range(3) for r2 in range(3))


def _two_shared(fam):
    rng = np.random.default_rng(107)
    for trial in range(2):
        a, b, c = rng.uniform(-2.0, 2.0, (3, 3))
        t1 = T(a, b, c)
        wa, wb = rng.uniform(0.1, 0.45, 2)
        ax = int(np.argmax(np.abs(np.cross(b - a, c - a))))
        on_edge = a + wa * (b - a)
        places = (("folded", on_edge + wb * (c - a)), ("flat", on_edge - wb * (c - a)),
                  ("beyond", a + 1.3 * (b - a) + 0.4 * (c - a)),
                  ("beside_in", on_edge + 2.0 ** -20 * (c - a)), ("beside_out", on_edge - 2.0 ** -20 * (c - a)))
        for kind, base in places:
            for i, val in enumerate(_steps(float(base[ax]), 4.0)):
                p = _moved(base, ax, val)
                for j in range(3):
                    r1, r2, wind = TWO_SHARED_COMBOS[(3 * i + j) % 18]
                    t2 = T(b, a, p) if wind == 0 else T(a, b, p)
                    fam.add(_rot(t1, r1), _rot(t2, r2), kind, 2)


def _sliver(fam):
    rng = np.random.default_rng(109)
    for trial in range(3):
        a, b = rng.uniform(-2.0, 2.0, (2, 3))
        up = np.cross(b - a, rng.uniform(-1.0, 1.0, 3))
        up /= np.linalg.norm(up)                                          # across the long edge
        d = rng.uniform(-1.0, 1.0, 3)
        s, u = rng.uniform(0.4, 1.0, 2)
        off = rng.uniform(-1.0, 1.0, 3)
        for e in (20, 30, 40, 50):
            t1 = T(a, b, 0.5 * (a + b) + 2.0 ** -e * up)
            for w in (0.3, 0.5):
                for o in SLIVER_OFFSETS:
                    y = a + w * (b - a) + o * up                          # where the partner's edge meets the sliver's plane
                    for side, far in (("near", y + off), ("away", y - off)):
                        t2 = T(y - s * d, y + u * d, far)
                        fam.add(t1, t2, "2^-%d_%s" % (e, side), 0)
                        fam.add(t2, t1, "2^-%d_%s" % (e, side), 0)


def _lattice(fam):
    rng = np.random.default_rng(31)
    for _ in range(1500):
        v = rng.integers(-2, 3, (6, 3)).astype(np.float64)
        fam.add(T(*v[:3]), T(*v[3:]), "lattice")
    t = fam.cases[0][0]
    for order in itertools.permutations(range(3)):                        # three shared vertices: coincident
        fam.add(t, tuple(t[k] for k in order), "coincident", 3)


def _scale(case, k, family="scaled"):
    f = 2.0 ** k
    t1, t2 = (tuple(tuple(x * f for x in p) for p in t) for t in case[:2])
    return (t1, t2, case[2], case[3], family)


def _perm3(a, b, c, d):
    """The permanent of orient3d(a, b, c, d), to a few ulp: for aiming at the guard, not for deciding anything."""
    (ax, ay, az), (bx, by, bz), (cx, cy, cz) = ((p[0] - d[0], p[1] - d[1], p[2] - d[2]) for p in (a, b, c))
    return ((abs(bx * cy) + abs(cx * by)) * abs(az) + (abs(cx * ay) + abs(ax * cy)) * abs(bz)) + (abs(ax * by) + abs(bx * ay)) * abs(cz)


def _sum2(a, b, c):
    return abs((a[0] - c[0]) * (b[1] - c[1])) + abs((a[1] - c[1]) * (b[0] - c[0]))


def _permanents(case):
    """The permanents of the plane-sign calls of the rule: a face's corners in their order against each corner of the
    other face.  A rotation of the three corners changes the permanent by rounding alone."""
    t1, t2 = case[:2]
    return sorted({_perm3(*s, d) for s, t in ((t1, t2), (t2, t1)) for d in t})


def _detsums(case):
    """The detsums of the 2-D calls of the rule in the dominant projection of face 1: every edge of either face against
    every other corner of the pair.  The order of an edge's ends does not change the detsum."""
    ax = X.dominant_axis(*case[0])
    pts = [X.drop(p, ax) for p in case[0] + case[1]]
    out = set()
    for e in ((0, 1), (1, 2), (2, 0), (3, 4), (4, 5), (5, 3)):
        out |= {_sum2(pts[e[0]], pts[e[1]], pts[k]) for k in range(6) if k not in e}
    return sorted(out)


GUARD_MARGINS = (1.0 - 1e-4, 1.0 + 1e-4, 1.0 - 1e-9, 1.0 + 1e-9)
GUARD_EVERY = 16                                        # every sixteenth case of the subset
GUARD_2D_PER_KIND = 2


def _apart(rng):
    """Two faces without a shared vertex whose projections along any axis are apart."""
    a, b, c = rng.uniform(-2.0, 2.0, (3, 3))
    return make_case(T(a, b, c), T(a + 5.0, b + 5.0, c + 5.0), "scaled", 0)


def _guard_2d_bases():
    """Pairs that the 2-D tests prove disjoint once every orient3d is uncertain: what `subset` leaves out, and a pair
    that lies apart."""
    out = []
    for name, kind in (("corner", "wedge"), ("two_shared", "flat"), ("two_shared", "beside_out"), ("one_shared_edge", "at_corner")):
        at = [i for i, k in enumerate(kinds(name)) if k == kind]
        out += [family(name)[at[(2 * n + 1) * len(at) // (2 * GUARD_2D_PER_KIND)]] for n in range(GUARD_2D_PER_KIND)]
    rng = np.random.default_rng(113)
    return out + [_apart(rng) for _ in range(GUARD_2D_PER_KIND)]


def _guard(fam):
    """Cases times a factor, not a power of two, that puts one value within 1e-4 and within 1e-9 of 2^-900 on either
    side.  guard_3d: a permanent of a plane-sign call, at about 2^-300, over every sixteenth case of the subset.
    guard_2d: a detsum, at about 2^-450, where every orient3d is uncertain and the 2-D tests decide, over pairs that
    those tests prove disjoint -- with the detsum of the separating edge below the guard they no longer do.  The kind is
    "guard_3d:g:m" / "guard_2d:g:m": group g holds one base and one value under the four margins m."""
    group = 0
    for dim, k, power, bases, values in (("3d", -300, 3, subset()[::GUARD_EVERY], _permanents),
                                         ("2d", -450, 2, _guard_2d_bases(), _detsums)):
        for case in bases:
            small = _scale(case, k)
            for value in values(small):
                if not (0.0 < value < INF):
                    continue
                for m, margin in enumerate(GUARD_MARGINS):
                    f = (X.TINY * margin / value) ** (1.0 / power)
                    t1, t2 = (tuple(tuple(x * f for x in p) for p in t) for t in small[:2])
                    fam.add(t1, t2, "guard_%s:%d:%d" % (dim, group, m))
                group += 1


def _scaled(fam):
    for k in SCALES_SAME + SCALES_SOUND:
        for case in subset():
            fam.cases.append(_scale(case, k))
            fam.kinds.append("2^%d" % k)
    _guard(fam)


def _shifted(fam):
    for shift in SHIFTS:
        for case in subset():
            t1, t2 = (T(*(np.array(t) + shift)) for t in case[:2])
            fam.add(t1, t2, "+2^%d" % int(np.log2(shift)))


_BUILDERS = {"corner": _corner, "edge_edge": _edge_edge, "one_shared_edge": _one_shared_edge, "two_shared": _two_shared,
             "sliver": _sliver, "scaled": _scaled, "shifted": _shifted, "lattice": _lattice}


@functools.lru_cache(maxsize=None)
def _family(name):
    fam = _Family(name)
    _BUILDERS[name](fam)
    return tuple(fam.cases), tuple(fam.kinds)


def family(name):
    """The cases of a family, built once a process."""
    return _family(name)[0]


def kinds(name):
    return _family(name)[1]


@functools.lru_cache(maxsize=None)
def _subset():
    out = []
    for name in BUILT:
        ok = [i for i, k in enumerate(kinds(name)) if k not in OFF_SUBSET]
        out += [(name, i) for i in ok[::-(-len(ok) // SUBSET_PER_FAMILY)]]
    return tuple(out)


def subset():
    """The cases that are scaled and shifted: SUBSET_PER_FAMILY of each constructed family, evenly spaced."""
    return tuple(family(name)[i] for name, i in _subset())


def scaled(k):
    """subset() times 2^k, case by case."""
    n, ks = len(_subset()), SCALES_SAME + SCALES_SOUND
    at = ks.index(k)
    return family("scaled")[at * n:(at + 1) * n]


def guard_cases():
    """The cases of the scaled family that aim at the 2^-900 guard: what follows the blocks of `scaled(k)`."""
    return family("scaled")[len(_subset()) * len(SCALES_SAME + SCALES_SOUND):]


def meets(t1, t2, id1, id2):
    """The oracle's answer for two faces.  It is a function of the two sets of corners and of which corners are shared,
    so it is remembered under a key that forgets the order of the corners in a face and the order of the faces."""
    f1 = tuple(sorted(zip(t1, (i in id2 for i in id1))))
    f2 = tuple(sorted(zip(t2, (i in id1 for i in id2))))
    return _meets(*sorted((f1, f2)))


@functools.lru_cache(maxsize=None)
def _meets(f1, f2):
    # ids with the same pattern of membership: corner k of face 1 is k, a shared corner of face 2 takes the id of the
    # corner of face 1 with its coordinates, every other corner 3 + k
    t1, t2 = tuple(p for p, _ in f1), tuple(p for p, _ in f2)
    id2 = tuple(t1.index(p) if s else 3 + k for k, (p, s) in enumerate(f2))
    assert tuple(i in id2 for i in (0, 1, 2)) == tuple(s for _, s in f1)
    return oracle(t1, t2, (0, 1, 2), id2)


@functools.lru_cache(maxsize=None)
def states(name):
    """The checker's (state, coincident) of every case of a family, once a process."""
    return tuple(X.pair_state(*c[:4]) for c in family(name))


def boxes_meet(t1, t2):
    """The box step of the rule: closed boxes with a common point."""
    return all(min(p[k] for p in t1) <= max(p[k] for p in t2) and min(p[k] for p in t2) <= max(p[k] for p in t1)
               for k in range(3))


def rule_state(t1, t2, id1=(0, 1, 2), id2=(3, 4, 5)):
    """The state of a pair of proper faces in a mesh: disjoint by the box step, else the narrow phase's."""
    return X.pair_state(t1, t2, id1, id2)[0] if boxes_meet(t1, t2) else D


def counts(values):
    """[disjoint, intersecting, undecided] of a sequence of states or of (state, coincident)."""
    out = [0, 0, 0]
    for s in values:
        out[s[0] if isinstance(s, tuple) else s] += 1
    return out


# ---- cases as meshes -----------------------------------------------------------------------------------------------------

def pack(cases):
    """The cases as one mesh, six vertices and two faces a case: case k is the faces 2 k and 2 k + 1."""
    v = np.array([c[0] + c[1] for c in cases], dtype=np.float64).reshape(-1, 3)
    return v, np.arange(len(v), dtype=np.int64).reshape(-1, 3)


def pack_two(cases, swapped=False):
    """The first faces as mesh a and the second as mesh b (swapped: the other way round): case k is the pair (k, k)."""
    a, b = ((1, 0) if swapped else (0, 1))
    va = np.array([c[a] for c in cases], dtype=np.float64).reshape(-1, 3)
    vb = np.array([c[b] for c in cases], dtype=np.float64).reshape(-1, 3)
    f = np.arange(len(va), dtype=np.int64).reshape(-1, 3)
    return va, f, vb, f


def batches(name):
    """A family in runs of at most BATCH_CASES cases.  The scaled family is cut at the ends of its blocks, so that no mesh
    mixes two scales: a batch a power of two, then the guard cases of either kind in runs."""
    if name == "scaled":
        g = guard_cases()
        n3 = sum(k.startswith("guard_3d") for k in kinds(name))
        runs = [scaled(k) for k in SCALES_SAME + SCALES_SOUND]
        for part in (g[:n3], g[n3:]):
            runs += [part[k:k + BATCH_CASES] for k in range(0, len(part), BATCH_CASES)]
        return runs
    c, n = family(name), BATCH_CASES_OF.get(name, BATCH_CASES)
    return [c[k:k + n] for k in range(0, len(c), n)]


# ---- the box step at equality ----------------------------------------------------------------------------------------------

TOUCHING = 256                                          # faces a group: one chunk each


TOUCHING_MESHES = [(1.0, False, 0), (0.0, True, 0), (1.0, False, 1), (1.0, False, 2)]      # (at, signed_zeros, axis)
TOUCHING_IDS = ["x_at_one", "x_at_signed_zeros", "y_at_one", "z_at_one"]


def touching_mesh(at=1.0, signed_zeros=False, axis=0):
    """512 faces whose only near pairs touch in one value of x (axis 1, 2: the coordinates moved on, so that what is
    said of x here holds of y, of z, and the slabs go along that axis).  Face k < 256 reaches from x = at - 301 to its corner
    (at, y, 0), y = k / 2; face 256 + k lies in the plane x = at and holds that corner strictly inside.  The boxes of the
    two faces share the value x = at alone, and so do the boxes of the two chunks the slab order along x makes of the
    groups.  signed_zeros (with at = 0): the value is written -0.0 in the first group and +0.0 in the second."""
    assert not signed_zeros or at == 0.0
    lo, hi = (-0.0, 0.0) if signed_zeros else (at, at)
    v = []
    for k in range(TOUCHING):
        y = 0.5 * k
        v += [(at - 301.0, y, 0.0), (lo, y, 0.0), (at - 151.0, y + 0.25, 0.25)]
    for k in range(TOUCHING):
        y = 0.5 * k
        v += [(hi, y - 0.125, -0.125), (hi, y + 0.125, -0.125), (hi, y, 0.25)]
    v = np.roll(np.array(v, dtype=np.float64), axis, axis=1)
    return v, np.arange(len(v), dtype=np.int64).reshape(-1, 3)


def rounding_degenerate_mesh():
    """A crossing pair and, inside face 0 and in its plane, a face whose corners are 2^-600 apart: its exact normal is
    2^-1200, the rounded one exactly zero, so the rule counts it as degenerate and tests it against nothing."""
    t = 2.0 ** -600
    v = np.array([(-1, -1, 0), (3, -1, 0), (-1, 3, 0), (0.5, 0.5, -1), (0.5, 0.5, 1), (1.5, 1, 1), (0, 0, 0), (t, 0, 0), (0, t, 0)],
                 dtype=np.float64)
    return v, np.arange(9, dtype=np.int64).reshape(-1, 3)
