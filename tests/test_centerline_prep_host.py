"""The centerline's branch structure without a device: csrc/mm_cl_branches.cpp (through ``Centerline``'s methods) and the
checker (tests/mm_checkers/centerline_prep.py) against

* the known answers of the reference's own tests (centerline_tests, src/types/native/centerline.rs:1022-1524), restated as
  data: sharp angles, split, merge, tangents, overlap removal, trimming, both orientations, and the four smoothing
  properties it asserts.  The reference holds no test of calculate_branches, and of smooth only those properties (no
  value): for these two, parity rests on the checker;
* each other, bit for bit (coordinates, radius, branch ids, branch start indices, tangents), on seeded synthetic trees
  written the way a CSV export writes them (segments one after the other, with jumps) and the way a VTP export does
  (every side branch repeats the prefix it shares with the main vessel), and on hypothesis cases;
* the properties calculate_branches' documentation promises;
* prepare_centerline's order of steps and skip rules; the mask-to-lists selection of label_branches (mm_branch_select)
  against the checker's.
"""
import math
import os

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings, strategies as st

from mm_checkers import centerline_prep as K

import multimoda_rs_amd as mm

N = mm._native
CLD = mm.centerline.CL_DTYPE
SET = dict(deadline=None, derandomize=True, database=None,
           suppress_health_check=[HealthCheck.function_scoped_fixture, HealthCheck.too_slow])
SCALE = int(os.environ.get("MM_HYP_SCALE", "1"))


# ---- the two implementations behind one face -----------------------------------------------------------------------------

def to_mm(c: K.CL) -> mm.Centerline:
    a = np.zeros(len(c.pts), dtype=CLD)
    for i, (p, b, t) in enumerate(zip(c.pts, c.branch_id, c.tangents)):
        a[i] = (p[0], p[1], p[2], t[0], t[1], t[2], p[3], b, 0)
    return mm.Centerline(a)


class Host:
    name = "host"
    make, from_coords = staticmethod(lambda br: to_mm(K.CL.from_branches(br))), staticmethod(lambda c: to_mm(K.CL.from_coords(c)))
    calculate_branches = staticmethod(lambda c, t: c.calculate_branches(t))
    find_sharp_angles = staticmethod(lambda c, b, t: c.find_sharp_angles(b, t))
    split_branch = staticmethod(lambda c, b, i: c.split_branch(b, i))
    merge_branches = staticmethod(lambda c, a, b: c.merge_branches(a, b))
    orient_by_max_z = staticmethod(lambda c: c.orient_by_max_z())
    orient_to_reference = staticmethod(lambda c, r: c.orient_to_reference(r))
    remove_branch_overlap = staticmethod(lambda c: c.remove_branch_overlap())
    trim_start = staticmethod(lambda c, m: c.trim_start(m))
    smooth = staticmethod(lambda c, s: c.smooth(s))
    resample = staticmethod(lambda c, s: c.resample(s))
    starts = staticmethod(lambda c: list(c.branch_start_indices))
    xyz = staticmethod(lambda c: [tuple(float(v) for v in r) for r in c.xyz()])
    ids = staticmethod(lambda c: [int(b) for b in c.points["branch_id"]])
    tangents = staticmethod(lambda c: [(float(p["tx"]), float(p["ty"]), float(p["tz"])) for p in c.points])


class Checker:
    name = "checker"
    make, from_coords = staticmethod(K.CL.from_branches), staticmethod(K.CL.from_coords)
    calculate_branches, find_sharp_angles = staticmethod(K.calculate_branches), staticmethod(K.find_sharp_angles)
    split_branch, merge_branches = staticmethod(K.split_branch), staticmethod(K.merge_branches)
    orient_by_max_z, orient_to_reference = staticmethod(K.orient_by_max_z), staticmethod(K.orient_to_reference)
    remove_branch_overlap, trim_start = staticmethod(K.remove_branch_overlap), staticmethod(K.trim_start)
    smooth, resample = staticmethod(K.smooth), staticmethod(K.resample)
    starts = staticmethod(lambda c: list(c.starts))
    xyz = staticmethod(lambda c: [p[:3] for p in c.pts])
    ids = staticmethod(lambda c: list(c.branch_id))
    tangents = staticmethod(lambda c: list(c.tangents))


IMPLS = [Checker, Host]


def lens(I, c):
    s = I.starts(c) + [len(I.xyz(c))]
    return [b - a for a, b in zip(s, s[1:])]


def branches(I, c):
    s = I.starts(c) + [len(I.xyz(c))]
    return [I.xyz(c)[a:b] for a, b in zip(s, s[1:])]


def line(n, y=0.0, x0=0):
    return [(float(x0 + i), y, 0.0) for i in range(n)]


V_SHAPE = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (2.0, 0.0, 0.0), (3.0, 0.0, 0.0), (2.5, 0.5, 0.0), (2.0, 1.0, 0.0)]


# ---- the reference's own tests, restated (centerline.rs:1022-1524) --------------------------------------------------------

@pytest.mark.parametrize("I", IMPLS, ids=lambda i: i.name)
class TestReferenceKnownAnswers:
    def test_find_sharp_angles(self, I):
        assert I.find_sharp_angles(I.from_coords(line(5)), 0, 0.0) == []
        v = I.from_coords(V_SHAPE)
        assert I.find_sharp_angles(v, 0, 0.0) == [3]
        assert I.find_sharp_angles(v, 0, 0.8) == []
        assert I.find_sharp_angles(v, 5, 0.0) == []
        two = I.make([[(0., 0., 0.), (0., 0., 1.), (0., 0., 2.)], V_SHAPE])
        assert I.find_sharp_angles(two, 1, 0.0) == [6]                      # a global index, not a position in the branch

    def test_split_branch(self, I):
        c = I.split_branch(I.from_coords(line(9)), 0, 3)
        assert lens(I, c) == [6, 4] and I.ids(c) == [0] * 6 + [1] * 4       # the longer piece is branch 0
        c = I.split_branch(I.from_coords(line(5)), 0, 2)
        assert I.starts(c) == [0, 3]                                        # equal pieces: the first stays the main
        c = I.split_branch(I.make([line(5), line(5, x0=10)]), 1, 7)         # point_index 7 = position 2 of branch 1
        b = branches(I, c)
        assert [len(x) for x in b] == [5, 3, 3] and b[1][0][0] == 10.0 and b[2][0][0] == 12.0
        c = I.split_branch(I.make([line(10), line(6, 1.0), line(2, 2.0)]), 1, 13)
        assert lens(I, c) == [10, 4, 3, 2]                                  # both pieces sort ahead of the shorter branch

    def test_merge_branches(self, I):
        c = I.merge_branches(I.split_branch(I.from_coords(line(5)), 0, 2), 0, 1)
        assert I.starts(c) == [0] and len(I.xyz(c)) == 6 and set(I.ids(c)) == {0}
        side1 = [(0., 1., 0.), (1., 1., 0.), (2., 1., 0.), (3., 1., 0.)]
        side2 = [(3., 1., 0.), (4., 1., 0.), (5., 1., 0.), (6., 1., 0.)]
        c = I.merge_branches(I.make([line(5), side1, side2]), 1, 2)
        assert lens(I, c) == [8, 5]                                         # the merged branch is now the longest: branch 0

    def test_tangents(self, I):
        assert I.tangents(I.from_coords(line(3))) == [(1.0, 0.0, 0.0)] * 3

    def test_remove_branch_overlap(self, I):
        side = [(0., 0., 0.), (1., 0., 0.), (2., 0., 0.), (2., 1.5, 0.), (2., 3., 0.)]
        b = branches(I, I.remove_branch_overlap(I.make([line(5), side])))
        assert [len(x) for x in b] == [5, 3] and b[1][0] == (2.0, 0.0, 0.0)     # the junction and the two diverged points
        c = I.remove_branch_overlap(I.make([line(3), line(2)]))
        assert I.starts(c) == [0]                                           # a branch that never leaves the main is dropped
        c = I.remove_branch_overlap(I.make([line(3), [(0., 5., 0.), (0., 6., 0.), (0., 7., 0.)]]))
        assert lens(I, c) == [3, 3]

    def test_trim_start(self, I):
        c = I.trim_start(I.make([line(6)]), 3.0)
        assert I.starts(c) == [0] and len(I.xyz(c)) == 3 and I.xyz(c)[0][0] == 3.0

    def test_orient_by_max_z(self, I):
        up = [(0., 0., 0.), (0., 0., 1.), (0., 0., 2.)]
        b = branches(I, I.orient_by_max_z(I.make([up, [(0., 0., 2.), (5., 0., 2.)]])))
        assert b[0][0][2] == 2.0 and b[0][2][2] == 0.0 and b[1][0][0] == 0.0 and b[1][1][0] == 5.0
        assert I.xyz(I.orient_by_max_z(I.from_coords(up[::-1])))[0][2] == 2.0
        b = branches(I, I.orient_by_max_z(I.make([up, [(5., 0., 2.), (0., 0., 2.)]])))
        assert b[0][0][2] == 2.0 and b[1][0][0] == 0.0 and b[1][1][0] == 5.0

    def test_orient_to_reference(self, I):
        main = [(0., 0., 0.), (5., 0., 0.), (10., 0., 0.)]
        ref = I.from_coords([(10., 1., 0.), (20., 1., 0.)])
        b = branches(I, I.orient_to_reference(I.make([main, [(0., 0., 0.), (0., 5., 0.)]]), ref))
        assert b[0][0][0] == 10.0 and b[0][2][0] == 0.0 and b[1][0][0] == 0.0 and b[1][1][1] == 5.0
        assert I.xyz(I.orient_to_reference(I.from_coords(main[::-1]), ref))[0][0] == 10.0
        ref2 = I.make([[(0., 1., 0.), (1., 1., 0.)], [(10., 1., 0.), (11., 1., 0.)]])      # its side branch is not measured against
        assert I.xyz(I.orient_to_reference(I.from_coords(main), ref2))[0][0] == 0.0
        b = branches(I, I.orient_to_reference(I.make([main, [(10., 5., 0.), (0., 5., 0.)]]),
                                              I.from_coords([(0., 1., 0.), (-10., 1., 0.)])))
        assert b[0][0][0] == 0.0 and b[1][0][0] == 0.0 and b[1][1][0] == 10.0
        ref3 = I.make([[(0., 1., 0.), (1., 1., 0.)], [(10., 5., 0.), (11., 5., 0.)]])
        assert branches(I, I.orient_to_reference(I.make([main, [(0., 0., 0.), (10., 5., 0.)]]), ref3))[1][0][0] == 0.0

    def test_smooth_properties(self, I):
        straight = I.from_coords(line(20))
        for a, b in zip(I.xyz(straight), I.xyz(I.smooth(straight, 3.0))):
            assert max(abs(x - y) for x, y in zip(a, b)) < 1e-10
        pts = line(15)
        pts[7] = (7.0, 5.0, 0.0)
        assert 0.0 < I.xyz(I.smooth(I.from_coords(pts), 2.0))[7][1] < 5.0   # the spike is damped, not erased
        pts = line(20)
        pts[10] = (10.0, 3.0, 0.0)
        for t in I.tangents(I.smooth(I.from_coords(pts), 2.0)):
            ln = math.sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2])
            assert abs(ln - 1.0) < 1e-10 or ln < 1e-12
        c = I.from_coords(line(10))
        s = I.smooth(c, 0.0)
        assert I.xyz(s) == I.xyz(c) and I.tangents(s) == I.tangents(c) and I.ids(s) == I.ids(c)

    def test_resample_keeps_branches_apart(self, I):
        c = I.resample(I.from_coords([(0., 0., 0.), (10., 0., 0.)]), 2.5)
        assert [p[0] for p in I.xyz(c)] == [0.0, 2.5, 5.0, 7.5, 10.0]
        c = I.resample(I.make([[(0., 0., 0.), (10., 0., 0.)], [(10., 0., 0.), (10., 5., 0.)]]), 2.0)
        assert len(I.starts(c)) == 2 and branches(I, c)[1][0][1] == 0.0


# ---- synthetic trees -------------------------------------------------------------------------------------------------------

def tree(rng, n_side, spacing=0.5):
    """A main vessel and n_side side branches as point lists; side branch k leaves main point at[k] (its first point lies
    one step off that point)."""
    n_main = int(rng.integers(40, 90))
    d = np.array([0.3, 0.2, -1.0])
    p = np.array([10.0, -5.0, 80.0])
    main = []
    for _ in range(n_main):
        main.append(tuple(float(v) for v in p))
        d = d + 0.08 * rng.standard_normal(3)
        d /= np.linalg.norm(d)
        p = p + spacing * (1.0 + 0.2 * rng.uniform(-1, 1)) * d
    sides, at = [], []
    for _ in range(n_side):
        k = int(rng.integers(5, n_main - 5))
        u = np.cross(np.array(main[k + 1]) - np.array(main[k]), rng.standard_normal(3))
        u /= np.linalg.norm(u)
        q = np.array(main[k])
        br = []
        for _ in range(int(rng.integers(6, 40))):
            q = q + spacing * (1.0 + 0.2 * rng.uniform(-1, 1)) * u
            u = u + 0.05 * rng.standard_normal(3)
            u /= np.linalg.norm(u)
            br.append(tuple(float(v) for v in q))
        sides.append(br)
        at.append(k)
    return main, sides, at


def csv_style(rng, main, sides, artefact=False):
    """One unbranched point list: the main vessel (possibly cut in two pieces written in the other order), then every side
    branch after a jump, optionally a three-point speck far away."""
    cut = int(rng.integers(10, len(main) - 10))
    segs = [main[cut:], main[:cut]] if rng.integers(0, 2) else [main]
    segs += [s[::-1] if rng.integers(0, 2) else s for s in sides]
    if artefact:
        segs.append([(500.0 + 0.4 * i, 500.0, 500.0) for i in range(3)])
    return K.CL.from_coords([p for s in segs for p in s])


def vtp_style(main, sides, at):
    """Branches as a VTP export lists them: every side branch starts at the origin of the main vessel."""
    br = sorted([main] + [main[:k + 1] + s for s, k in zip(sides, at)], key=lambda b: -len(b))
    return K.CL.from_branches(br)


def bits(x):
    """Bit patterns, every NaN as one (the tangent of two coincident points is 0 / 0: its sign and payload say nothing)."""
    x = np.array(x, dtype=np.float64)
    x[np.isnan(x)] = np.nan
    return x.view(np.uint64)


def assert_same(h: mm.Centerline, k: K.CL):
    assert len(h) == len(k.pts)
    assert list(h.branch_start_indices) == list(k.starts)
    assert [int(b) for b in h.points["branch_id"]] == list(k.branch_id)
    kp = np.array(k.pts, dtype=np.float64).reshape(-1, 4)
    kt = np.array(k.tangents, dtype=np.float64).reshape(-1, 3)
    for col, name in enumerate(("x", "y", "z", "radius")):
        assert np.array_equal(bits(h.points[name]), bits(kp[:, col])), name
    for col, name in enumerate(("tx", "ty", "tz")):
        assert np.array_equal(bits(h.points[name]), bits(kt[:, col])), name


def arc(pts):
    return sum(K.dist(a, b) for a, b in zip(pts, pts[1:]))


@pytest.mark.parametrize("n_side", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_calculate_branches_on_csv_style_trees(seed, n_side):
    rng = np.random.default_rng(1000 * seed + n_side)
    main, sides, _ = tree(rng, n_side)
    raw = csv_style(rng, main, sides, artefact=bool(seed % 2))
    k = K.calculate_branches(raw, 2.0)
    h = to_mm(raw).calculate_branches(2.0)
    assert_same(h, k)
    # what the documentation promises
    got = k.branches()
    flat = [p for b in got for p in b]
    assert len(set(flat)) == len(flat) and set(flat) <= set(raw.pts)         # a selection of the input, nothing twice
    assert not any(p[0] >= 500.0 for p in flat)                             # the speck of 3 points is gone
    assert len(raw.pts) - len(flat) - (3 if seed % 2 else 0) <= 4 * n_side  # beside it only leftovers of fewer than 5 points
    assert [len(b) for b in got[1:]] == sorted((len(b) for b in got[1:]), reverse=True)
    assert all(len(b) >= 5 for b in got[1:])
    # branch 0 is the longest path by arc length: no branch is longer, and the main vessel as generated (a path of the
    # tree: its two pieces join where they were cut) is not longer either -- a long side branch may take over its far end
    assert all(arc(got[0]) >= arc(b) for b in got[1:]) and arc(got[0]) >= arc(main) - 1e-9
    ends = {got[0][0][:3], got[0][-1][:3]}
    assert ends <= {main[0], main[-1]} | {s[-1] for s in sides}             # it runs from one tip of the tree to another
    assert list(h.branch_start_indices) == list(np.flatnonzero(np.diff(h.points["branch_id"], prepend=-1)))   # ids run 0, 1, ...
    for b in got[1:]:                                                       # each side branch is walked as a chain
        assert max(K.dist(p, q) for p, q in zip(b, b[1:])) < 2.0 * 0.5 * 1.2 * 1.01


@pytest.mark.parametrize("n_side", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("seed", [4, 5])
def test_every_method_on_vtp_style_trees(seed, n_side):
    rng = np.random.default_rng(77 * seed + n_side)
    main, sides, at = tree(rng, n_side)
    k0 = vtp_style(main, sides, at)
    h0 = to_mm(k0)
    ref = K.CL.from_coords([(0.0, 0.0, 120.0 - i) for i in range(40)])
    k1, h1 = K.remove_branch_overlap(k0), h0.remove_branch_overlap()
    assert_same(h1, k1)
    assert len(k1.starts) == 1 + n_side
    buf, known = K.mean_spacing(k0), list(k1.branches()[0])
    for b in k1.branches()[1:]:                 # the junction (the last point within the buffer) stays, the prefix goes
        assert min(K.dist(b[0], m) for m in known) <= buf < min(K.dist(b[1], m) for m in known)
        known += b
    for kk, hh in ((K.trim_start(k1, 3.3), h1.trim_start(3.3)), (K.orient_by_max_z(k1), h1.orient_by_max_z()),
                   (K.orient_to_reference(k1, ref), h1.orient_to_reference(to_mm(ref))),
                   (K.smooth(k1, 2.5), h1.smooth(2.5)), (K.smooth(k1, 0.4), h1.smooth(0.4)),
                   (K.resample(k1, 0.8), h1.resample(0.8))):
        assert_same(hh, kk)
    nb = len(k1.starts)
    for b in range(nb):
        assert h1.find_sharp_angles(b, 0.9 - 1.0) == K.find_sharp_angles(k1, b, 0.9 - 1.0)
        mid = k1.starts[b] + 3
        assert_same(h1.split_branch(b, mid), K.split_branch(k1, b, mid))
        assert_same(h1.split_branch(b, k1.starts[b]), K.split_branch(k1, b, k1.starts[b]))     # at an end: unchanged
    for a in range(nb):
        for b in range(nb):
            assert_same(h1.merge_branches(a, b), K.merge_branches(k1, a, b))


@settings(max_examples=40 * SCALE, **SET)
@given(seed=st.integers(0, 2**31 - 1), n_side=st.integers(0, 4), tol=st.sampled_from([1.2, 2.0, 3.5]),
       sigma=st.sampled_from([0.3, 1.0, 2.5, 7.0]), artefact=st.booleans(), grid=st.booleans())
def test_host_equals_checker_on_generated_trees(seed, n_side, tol, sigma, artefact, grid):
    rng = np.random.default_rng(seed)
    main, sides, at = tree(rng, n_side, spacing=float(rng.choice([0.25, 0.5, 1.0])))
    if grid:        # coordinates on a coarse grid: equal distances, coincident points, exact ties
        main = [tuple(round(v * 2) / 2 for v in p) for p in main]
        sides = [[tuple(round(v * 2) / 2 for v in p) for p in s] for s in sides]
    raw = csv_style(rng, main, sides, artefact)
    k, h = K.calculate_branches(raw, tol), to_mm(raw).calculate_branches(tol)
    assert_same(h, k)
    assert_same(h.smooth(sigma), K.smooth(k, sigma))
    assert_same(h.orient_by_max_z(), K.orient_by_max_z(k))
    v = vtp_style(main, sides, at)
    assert_same(to_mm(v).remove_branch_overlap(), K.remove_branch_overlap(v))
    t = float(rng.uniform(0, 8))
    assert_same(to_mm(v).trim_start(t), K.trim_start(v, t))


def test_degenerate_inputs():
    empty = mm.Centerline(np.zeros(0, dtype=CLD))
    for out in (empty.calculate_branches(2.0), empty.orient_by_max_z(), empty.remove_branch_overlap(), empty.smooth(2.0),
                empty.trim_start(1.0), empty.split_branch(0, 0), empty.merge_branches(0, 1), empty.orient_to_reference(empty)):
        assert len(out) == 0
    assert empty.find_sharp_angles(0, 0.0) == []
    two = to_mm(K.CL.from_coords([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0)]))
    assert_same(two.calculate_branches(2.0), K.calculate_branches(K.CL.from_coords([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0)]), 2.0))
    bad = two.points.copy()
    bad["x"][1] = np.nan
    with pytest.raises(RuntimeError):
        mm.Centerline(bad).calculate_branches(2.0)
    L = N.lib()
    assert L.mm_centerline_smooth(None, 3, 1.0, None) < 0 and L.mm_centerline_calculate_branches(None, -1, 2.0, None) < 0
    # a NaN sigma passes the `< 1e-12` gate and changes no position (every weight is NaN)
    c = to_mm(K.CL.from_coords(line(6)))
    assert_same(c.smooth(float("nan")), K.smooth(K.CL.from_coords(line(6)), float("nan")))


# ---- prepare_centerline ------------------------------------------------------------------------------------------------------

class Traced(mm.Centerline):
    """A Centerline that writes down which of its methods prepare_centerline calls."""
    log: list = []


def _traced(name):
    def f(self, *a):
        Traced.log.append(name)
        return Traced(getattr(mm.Centerline, name)(self, *a).points)
    return f


for _n in ("calculate_branches", "remove_branch_overlap", "trim_start", "resample", "orient_to_reference",
           "orient_by_max_z", "smooth"):
    setattr(Traced, _n, _traced(_n))


def run_prepare(c: K.CL, **kw):
    Traced.log = []
    ref = kw.pop("ref", None)
    out = mm.prepare_centerline(Traced(to_mm(c).points), None if ref is None else to_mm(ref), **kw)
    trace = []
    want = K.prepare_centerline(c, ref, kw.get("spacing_mm"), kw.get("branch_spacing_tolerance", 2.0),
                                kw.get("rm_start_mm", 0.0), kw.get("smooth_sigma", 2.5), trace=trace)
    assert Traced.log == trace
    assert_same(out, want)
    return trace


def test_prepare_centerline_steps_and_skips():
    rng = np.random.default_rng(5)
    main, sides, at = tree(rng, 2)
    raw, vtp = csv_style(rng, main, sides), vtp_style(main, sides, at)
    aorta = K.CL.from_coords([(0.0, 0.0, 60.0 + 0.7 * i) for i in range(60)])
    full = ["calculate_branches", "remove_branch_overlap", "trim_start", "resample", "orient_to_reference", "smooth"]
    assert run_prepare(raw, ref=aorta, spacing_mm=0.7, rm_start_mm=2.0) == full
    # an input that already has branches is not branched again
    assert run_prepare(vtp, ref=aorta, spacing_mm=0.7, rm_start_mm=2.0) == full[1:]
    # the aorta (no reference) is never branched and is oriented by its highest point
    assert run_prepare(aorta) == ["remove_branch_overlap", "orient_by_max_z", "smooth"]
    assert run_prepare(raw) == ["remove_branch_overlap", "orient_by_max_z", "smooth"]
    # each switch skips exactly its step
    assert run_prepare(raw, ref=aorta, rm_start_mm=0.0, spacing_mm=0.7) == [s for s in full if s != "trim_start"]
    assert run_prepare(raw, ref=aorta, rm_start_mm=2.0, spacing_mm=None) == [s for s in full if s != "resample"]
    assert run_prepare(raw, ref=aorta, rm_start_mm=2.0, spacing_mm=0.7, smooth_sigma=0.0) == full[:-1]
    assert run_prepare(raw, ref=aorta, smooth_sigma=0.0) == ["calculate_branches", "remove_branch_overlap", "orient_to_reference"]


def test_load_centerline(tmp_path, capsys):
    rng = np.random.default_rng(2)
    xyz = np.cumsum(rng.uniform(0.1, 0.5, (30, 3)), axis=0)
    c = mm.numpy_to_centerline(xyz)
    assert mm.load_centerline(c, "RCA") is c
    assert np.array_equal(mm.load_centerline(xyz, "RCA").points, c.points)
    f = tmp_path / "cl.csv"
    np.savetxt(f, xyz, delimiter=",", fmt="%.17g")
    assert np.array_equal(mm.load_centerline(f, "LCA").points, c.points)
    assert np.array_equal(mm.load_centerline(str(f), "LCA").points, c.points)
    out = capsys.readouterr().out
    assert "Using provided RCA centerline: 30 points" in out and "Loaded LCA centerline: 30 points" in out
    with pytest.raises(Exception):
        mm.load_centerline(tmp_path / "missing.csv", "Aorta")
    assert "Error reading Aorta centerline" in capsys.readouterr().out
    with pytest.raises(RuntimeError):
        mm.load_centerline(tmp_path / "missing.vtp", "Aorta")


# ---- the lists of label_branches from masks (mm_branch_select) --------------------------------------------------------------

def host_select(masks, main_ids, n_branches, cap=None):
    masks = np.ascontiguousarray(masks, dtype=np.uint64)
    n = masks.shape[0]
    ids = np.array(main_ids, dtype=np.uint32)
    mi, si = np.zeros(max(n, 1), dtype=np.int64), np.zeros(max(n, 1), dtype=np.int64)
    off, counts = np.zeros(n_branches + 1, dtype=np.int64), np.zeros(3, dtype=np.int64)
    L = N.lib()
    N.check(L.mm_branch_select(N._ptr(masks), n, N._ptr(ids), len(ids), n_branches, N._ptr(mi), N._ptr(si), N._ptr(off),
                               None, 0, N._ptr(counts)))
    sk = np.zeros(max(int(counts[2]) if cap is None else cap, 1), dtype=np.int64)
    N.check(L.mm_branch_select(N._ptr(masks), n, N._ptr(ids), len(ids), n_branches, N._ptr(mi), N._ptr(si), N._ptr(off),
                               N._ptr(sk), int(counts[2]) if cap is None else cap, N._ptr(counts)))
    return mi[:counts[0]], si[:counts[1]], {k: sk[off[k]:off[k + 1]] for k in range(n_branches)}, counts


@settings(max_examples=60 * SCALE, **SET)
@given(seed=st.integers(0, 2**31 - 1), n=st.integers(0, 300), nb=st.integers(0, 64), n_main=st.integers(0, 3))
def test_select_equals_the_checker(seed, n, nb, n_main):
    rng = np.random.default_rng(seed)
    masks = np.zeros(n, dtype=np.uint64)
    for _ in range(3):                                                      # sparse masks: a few bits a point
        bit = rng.integers(0, max(nb, 1), n).astype(np.uint64)
        masks |= np.where(rng.uniform(size=n) < 0.4, np.uint64(1) << bit, np.uint64(0)).astype(np.uint64)
    main_ids = [int(b) for b in rng.integers(0, max(nb, 1), n_main)]
    m, s, sk, counts = host_select(masks, main_ids, nb)
    km, ks, ksk = K.select(masks, main_ids, nb)
    assert np.array_equal(m, km) and np.array_equal(s, ks)
    for k in range(nb):
        assert np.array_equal(sk[k], ksk.get(k, np.zeros(0, dtype=np.int64))), k
    assert counts[2] == sum(len(v) for v in ksk.values())


def test_select_reports_what_does_not_fit_and_rejects_bad_arguments():
    masks = np.array([2, 6, 1, 4], dtype=np.uint64)
    _, _, _, counts = host_select(masks, [0], 3, cap=1)
    assert list(counts) == [1, 3, 4]                                        # 4 entries needed, none written into 1 slot
    L = N.lib()
    c = np.zeros(3, dtype=np.int64)
    off = np.zeros(66, dtype=np.int64)
    ids = np.array([64], dtype=np.uint32)
    assert L.mm_branch_select(N._ptr(masks), 4, N._ptr(ids), 1, 3, None, None, N._ptr(off), None, 0, N._ptr(c)) < 0
    assert L.mm_branch_select(N._ptr(masks), 4, None, 0, 65, None, None, N._ptr(off), None, 0, N._ptr(c)) < 0
    assert L.mm_branch_select(None, 4, None, 0, 3, None, None, N._ptr(off), None, 0, N._ptr(c)) < 0
    assert L.mm_branch_masks(None, None, 0, None, 0, 1.0, None) < 0 and "engine" in N.last_error()
