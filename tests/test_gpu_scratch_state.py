"""Stale scratch never reaches a result.  Every CCTA entry point stages its work in the engine's grow-only buffers
(dev_pts, dev_raw, dev_lvl, the pinned host_pts and host_lvl), which Engine::ensure never clears: a call starts on what
the call before it left at the same offsets, and is right only because of its clears and guards ("Scratch
planes read without a clear").  Here every entry point runs on an input X four times -- on a fresh engine (R0); on a
second engine behind its twin Y (tests/scratch_twins.py: the counts of X, other content, so every stale word sits in the
plane that will read it and looks valid) (R1); behind a larger input B, so that X's planes lie inside B's leftovers
(R2); and behind another entry point that carves the same buffers otherwise (R3) -- and R0 .. R3 must be equal bit for
bit in every array and every report field, R0 must equal the checker as the entry point's own GPU test asserts it, the
twin's result must differ from R0 (the case is not vacuous) and report the same bytes_uploaded (the same carving).

The buffers are dirtied by real calls only (no fill hook, no memset with a constant): stale key tables are at most a
quarter full, stale indices are below the counts of an input the buffer was sized for, stale counts are ones a real call
produced, so a defect shows as a wrong value and not as a fault.  The cases form a ring: case k is dirtied by case
k + 1's call, so every entry point serves once as the dirtying call.

No report here holds a time.  Left out of the bit comparison are the fields that are no function of the input alone,
whatever the scratch held: items_run, items_skipped and items_skipped_step0 of the pruned triangle
searches, which depend on the order in which the checked items ran (test_gpu_relax.settled leaves them out for the same
reason), and winding_rounds, the rounds of a pointer jumping that reads links other lanes are moving (the GPU tests of
the stitching and the closing bound it, 1 < rounds <= 2 + log2 nf, as same_assembly and same_fill do here).

Shapes: meshes of 257 vertices (one past a workgroup) and of 1460 vertices / 2916 faces (an edge table above the
256-slot floor, several flip and refine passes) with B = every face cut in four (11664 faces: several 4096-item scan
tiles); point sets of 255, 256, 257 and 3001; 257 and 700 faces for the ray pass."""
import numpy as np
import pytest

from mm_checkers import centerline_prep as CP
from mm_checkers import close_mesh as CM
from mm_checkers import flip_edges as FE
from mm_checkers import label_coronary as LC
from mm_checkers import refine_mesh as R
from mm_checkers import rim_condition as RK
from mm_checkers import scale_coronary as SC
from mm_checkers import smooth_mesh as SMO
from mm_checkers import stitch_mesh as SK
from mm_checkers import surface_distance as S
from mm_checkers import trim_mesh as TM
from helpers import blob, to_oracle_cl
from scratch_twins import big, big_points, differences, twin, twin_points, uploads
from test_refine_host import same_bits, jitter, wound_tube
from test_flip_host import flipped, tube, refined_tube, refined_open_tube
from test_gpu_refine import bits_equal, same_refine
from test_gpu_flip import same_flip
from test_gpu_relax import same_relax
from test_gpu_surface import same_as_checker
from test_gpu_smooth import same_csr, TAUBIN10
from test_gpu_close import same_fill
from test_gpu_trim import same_results, labelled
from test_gpu_stitch import same_assembly, reversed_subset
from test_gpu_rim import check_split
from test_gpu_discretize import curved_tube, check_vessel
from test_gpu_morph import cl_of, random_case as morph_case
from test_gpu_morphometry import assert_matches, ring as contour_ring, KEYS as MEASURE_KEYS, PAIRS as MEASURE_PAIRS
from test_gpu_label import _cl, _random_scene
from test_gpu_branch_label import make_cl

import multimoda_rs_amd as mm
from multimoda_rs_amd import ccta
from multimoda_rs_amd.centerline import Centerline

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    import __graft_entry__ as ge
    ge.build()
    clean, dirty = mm.Engine(), mm.Engine()
    yield clean, dirty
    dirty.close()
    clean.close()


# ---- the cases ------------------------------------------------------------------------------------------------------------

class Case:
    """call(engine, x, request) -> result; check(engine, x, r0, request) asserts r0 against the checker."""

    def __init__(self, name, call, x, check, twin_of, big_of):
        self.name, self.call, self._x, self.check, self.twin_of, self.big_of = name, call, x, check, twin_of, big_of
        self._made = None

    @property
    def x(self):
        if self._made is None:
            self._made = self._x()
        return self._made


CASES = []
MESHES = {"tube": tube, "refined_tube": refined_tube}
OPEN_MESHES = {"open_tube": lambda: (wound_tube(15, 17)[0], wound_tube(15, 17)[1][:-30]), "refined_open_tube": refined_open_tube}


def mesh_of(make):
    def build():
        v, f = make()
        return np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(f, dtype=np.int64)
    return build


def mesh_case(name, call, check, shapes=MESHES):
    for shape, make in shapes.items():
        CASES.append(Case(f"{name}-{shape}", call, mesh_of(make), check, lambda m: twin(m[0], m[1], 1), lambda m: big(*m)))


def point_case(name, call, check, x, twin_of=None, big_of=None):
    CASES.append(Case(name, call, x, check,
                      twin_of or (lambda t: tuple(twin_points(a, 1 + k) for k, a in enumerate(t))),
                      big_of or (lambda t: tuple(big_points(a, k) for k, a in enumerate(t)))))


def every_third(nv):
    m = np.zeros(nv, dtype=bool)
    m[::3] = True
    return m


# -- flips

def call_valence(e, m, request):
    return mm.mesh_valence(m, engine=e)


def check_valence(e, m, r0, request):
    deg, border, info = r0
    wdeg, wborder, winfo = FE.valence(m[1], len(m[0]))
    assert deg.dtype == np.int32 and border.dtype == np.bool_ and np.array_equal(deg, wdeg) and np.array_equal(border, wborder)
    assert info == dict(n_edges=winfo["n_edges"], n_open_edges=winfo["n_open_edges"],
                        n_nonmanifold_edges=winfo["n_nonmanifold_edges"], n_inconsistent_edges=winfo["n_inconsistent_edges"],
                        deviation=winfo["deviation"], n_launches=3)


def flip_kw(kind, nv):
    return {"plain": {}, "pinned": {"pinned": every_third(nv)}, "one_pass": {"passes": 1}}[kind]


def flip_calls(kind):
    def call(e, m, request):
        return mm.flip_edges(m, engine=e, **flip_kw(kind, len(m[0])))

    def check(e, m, r0, request):
        want = None
        if kind == "plain":                                               # the checker's answer, computed once a session
            for name in ("tube", "refined_tube"):
                if np.array_equal(flipped(name)[1], m[1]) and same_bits(flipped(name)[0], m[0]):
                    want = flipped(name)[2:4]
        gf, rep = same_flip(m[0], m[1], e, want=want, **flip_kw(kind, len(m[0])))
        assert differences((gf, rep), (r0[0][1], r0[1])) == [] and same_bits(r0[0][0], m[0])
    return call, check


mesh_case("mesh_valence", call_valence, check_valence)
for _kind in ("plain", "pinned", "one_pass"):
    mesh_case(f"flip_edges_{_kind}", *flip_calls(_kind))


# -- refine

def call_edge_lengths(e, m, request):
    return mm.mesh_edge_lengths(m, engine=e)


def check_edge_lengths(e, m, r0, request):
    wedges, wlen_sq = R.edge_lengths(*m)
    assert np.array_equal(r0[0], wedges) and same_bits(r0[1], np.sqrt(wlen_sq))


def refine_target(m):
    return 0.4 if len(m[0]) < 1000 else 0.3


def call_refine(e, m, request):
    return mm.refine_mesh(m, refine_target(m), engine=e)


def check_refine(e, m, r0, request):
    got = same_refine(m[0], m[1], refine_target(m), e)
    assert differences(got, r0) == []


mesh_case("mesh_edge_lengths", call_edge_lengths, check_edge_lengths)
mesh_case("refine_mesh", call_refine, check_refine)


# -- relax and surface

def call_relax(e, m, request):
    return mm.relax_mesh(m, None, iterations=2, lamb=0.5, engine=e)


def check_relax(e, m, r0, request):
    gv, face, rep = same_relax(m, None, e, 2, 0.5)
    assert differences((gv, face, rep), (r0[0][0], r0[1], r0[2])) == [] and np.array_equal(r0[0][1], m[1])


def queries_of(m):
    v, f = m
    return np.ascontiguousarray(jitter(np.concatenate([v, v[::2] * 1.1, v[::3] * 0.7]), 23)[:513 if len(v) < 1000 else 1300])


def call_point_mesh(e, m, request):
    return mm.point_mesh_distance(queries_of(m), m, engine=e)


def check_point_mesh(e, m, r0, request):
    assert differences(same_as_checker(queries_of(m), m[0], m[1], e), r0) == []


def other_surface(m):
    return jitter(m[0], 4) * 1.02, m[1]


def call_hausdorff(e, m, request):
    return mm.surface_distance(m, other_surface(m), engine=e)


def check_hausdorff(e, m, r0, request):
    a, b = m, other_surface(m)
    for d, (src, dst) in ((r0.a_to_b, (a, b)), (r0.b_to_a, (b, a))):
        p, owner = mm.sample_mesh_surface(src, 1)
        sq, face, closest, _ = S.scan(p, dst[0], dst[1])
        k = int(np.argmax(sq))
        assert d.n == len(p) and d.argmax == k and d.face == face[k] and d.sample_face == owner[k]
        assert same_bits(d.max, np.sqrt(sq[k])) and same_bits(d.closest, closest[k])
        total, total_sq = 0.0, 0.0
        for x, y in zip(np.sqrt(sq).tolist(), sq.tolist()):
            total, total_sq = total + x, total_sq + y
        assert same_bits(d.mean, total / len(p)) and same_bits(d.rms, np.sqrt(total_sq / len(p)))
    assert r0.hausdorff == max(r0.a_to_b.max, r0.b_to_a.max) > 0.0
    assert r0.bytes_uploaded == r0.a_to_b.report["bytes_uploaded"] + r0.b_to_a.report["bytes_uploaded"]


mesh_case("relax_mesh", call_relax, check_relax)
mesh_case("point_mesh_distance", call_point_mesh, check_point_mesh)
mesh_case("surface_distance", call_hausdorff, check_hausdorff, {"tube": tube})


# -- smooth

def call_csr(e, m, request):
    return mm.mesh_adjacency_csr(m[1], len(m[0]), engine=e)


def check_csr(e, m, r0, request):
    assert differences(same_csr(m[1], len(m[0]), e), r0) == []


def band_of(m):
    return [len(m[0]) // 2, 5], 3


def call_rings(e, m, request):
    seeds, max_ring = band_of(m)
    return ccta.vertex_rings_info(m[1], seeds, max_ring, len(m[0]), engine=e)


def check_rings(e, m, r0, request):
    seeds, max_ring = band_of(m)
    wring, winfo = SMO.rings(m[1], len(m[0]), seeds, max_ring)
    assert r0[0].dtype == np.int32 and np.array_equal(r0[0], wring) and r0[1] == winfo and 0 < winfo["reached"] < len(m[0])


def call_smooth_band(e, m, request):
    return mm.smooth_mesh(m, TAUBIN10, band=band_of(m), engine=e)


def check_smooth_band(e, m, r0, request):
    seeds, max_ring = band_of(m)
    hand = SMO.rings(m[1], len(m[0]), seeds, max_ring)[0] < 0
    want, wrep = SMO.smooth(m[0], m[1], TAUBIN10, hand)
    (gv, gf), rep = r0
    assert same_bits(gv, want) and not same_bits(gv, m[0]) and same_bits(gv[hand], m[0][hand])
    for k in ("n_vertices", "n_faces", "n_edges", "n_isolated", "n_pinned", "max_degree", "steps_run", "launches"):
        assert rep[k] == wrep[k], (k, rep[k], wrep[k])
    for k in ("volume_before", "volume_after", "max_displacement_sq"):
        assert bits_equal(rep[k], wrep[k]), (k, rep[k], wrep[k])


def labels_of(m):
    r = np.random.default_rng(len(m[0]))                                  # bands of three labels, one vertex in twelve another:
    lab = (np.arange(len(m[0])) // 90 % 3).astype(np.uint8)               # the lone ones are outvoted
    lone = r.random(len(lab)) < 1.0 / 12.0
    lab[lone] = (lab[lone] + 1 + r.integers(0, 2, int(lone.sum()))) % 3
    return lab


def call_labels(e, m, request):
    return ccta.smooth_mesh_labels_info(labels_of(m), iterations=3, faces=m[1], engine=e)


def check_labels(e, m, r0, request):
    want, winfo = CM.smooth_labels(labels_of(m), CM.adjacency_of_faces(m[1], len(m[0])), 3)
    assert r0[0].dtype == np.uint8 and np.array_equal(r0[0], want) and winfo["n_flips"] > 0
    for k in winfo:
        assert r0[1][k] == winfo[k], k


mesh_case("mesh_adjacency_csr", call_csr, check_csr)
mesh_case("vertex_rings", call_rings, check_rings)
mesh_case("smooth_mesh_band", call_smooth_band, check_smooth_band)
mesh_case("smooth_mesh_labels", call_labels, check_labels)


# -- close, trim

def call_fill(e, m, request):
    return mm.fill_holes(m[0], m[1], True, engine=e)


def check_fill(e, m, r0, request):
    got = same_fill(m[0], m[1], e)
    assert differences(got, r0) == [] and got[2]["n_loops_filled"] == 2


def call_open_edges(e, m, request):
    return mm.open_boundary_edges(m[1], engine=e)


def check_open_edges(e, m, r0, request):
    assert np.array_equal(r0, TM.open_boundary_edges(m[1])) and len(r0) > 0


def rim_seeds(m):
    return set(TM.open_boundary_edges(m[1]).ravel().tolist())


def call_clean(e, m, request):
    return mm.clean_open_boundary(m[1], m[0], rim_seeds(m), 2, engine=e)


def check_clean(e, m, r0, request):
    wd, wr = TM.clean_open_boundary(m[1], m[0], rim_seeds(m), 2)
    assert r0[0].tolist() == wd and [r.tolist() for r in r0[1]] == wr and len(wr) == 2


def call_remove(e, m, request):
    return mm.remove_labeled_points_from_mesh(labelled(m[0], m[1], 3), "anomalous_points", 1, engine=e)


def check_remove(e, m, r0, request):
    same_results(r0, TM.remove_labeled_points_from_mesh(labelled(m[0], m[1], 3), "anomalous_points", 1))
    assert len(r0["mesh"][1]) < len(m[1])


mesh_case("fill_holes", call_fill, check_fill, OPEN_MESHES)
mesh_case("open_boundary_edges", call_open_edges, check_open_edges, OPEN_MESHES)
mesh_case("clean_open_boundary", call_clean, check_clean, OPEN_MESHES)
mesh_case("remove_labeled_points", call_remove, check_remove)


# -- stitch

def part_reversed(m):
    return reversed_subset(m[1], np.random.default_rng(len(m[1])).random(len(m[1])) < 0.3)


def call_winding(e, m, request):
    return mm.fix_mesh_winding(part_reversed(m), engine=e)


def check_winding(e, m, r0, request):
    g = part_reversed(m)
    assert r0.dtype == np.int64 and np.array_equal(r0, SK.fix_winding(g)[0]) and not np.array_equal(r0, g)


def call_assemble(e, m, request):
    return mm.assemble_mesh([(m[0], part_reversed(m))], 3, True, True, engine=e)


def check_assemble(e, m, r0, request):
    assert differences(same_assembly([(m[0], part_reversed(m))], e), r0) == []


mesh_case("fix_mesh_winding", call_winding, check_winding)
mesh_case("assemble_mesh", call_assemble, check_assemble)


# -- rim

def locate_queries(v, n):
    r = np.random.default_rng(n)
    by_x = np.argsort(v[:, 0], kind="stable")                             # chosen by place, not by label: a twin answers otherwise
    pts = v[by_x[r.integers(0, len(v), n)]].copy()
    pts[::7] += 100.0                                                     # absent
    return pts


def call_locate(e, m, request):
    return [ccta.locate_points(m[0], locate_queries(m[0], n), e) for n in (255, 256, 257, 3001)]


def check_locate(e, m, r0, request):
    for n, got in zip((255, 256, 257, 3001), r0):
        want = RK.locate_points(m[0], locate_queries(m[0], n))
        assert np.array_equal(got, want) and (want >= 0).any() and (want < 0).any()


def rim_of(m):
    """The rim of the open tube at its first ring, in the order the open edges chain, and the split counts to 40."""
    edges = TM.open_boundary_edges(m[1])
    rings = TM.order_boundary_rings(m[1], m[0], None, None)
    ring = min(rings, key=lambda r: min(r))
    counts, status, gap = RK.densify_plan(m[0][ring], 2 * len(ring) + 3)
    assert status == 1 and len(edges) > 0
    return list(ring), counts


def call_split(e, m, request):
    ring, counts = rim_of(m)
    return ccta.split_rim_edges(m[0], m[1], ring, counts, e)


def check_split_case(e, m, r0, request):
    ring, counts = rim_of(m)
    assert differences(check_split(e, m, ring, counts), r0) == [] and r0[3]["n_inserted"] == len(ring) + 3


def call_layers(e, m, request):
    seeds = rim_of(m)[0]
    return ccta.enforce_layer_gap_from_plane(m, seeds, m[0][seeds].mean(axis=0), np.array([0.0, 0.0, 1.0]), 0.1, 3, engine=e,
                                             return_info=True)


def check_layers(e, m, r0, request):
    seeds = rim_of(m)[0]
    (wv, _), wl, rings_run, _ = RK.enforce_layer_gap_from_plane(m, seeds, m[0][seeds].mean(axis=0), np.array([0.0, 0.0, 1.0]),
                                                                0.1, 3)
    (gv, gf), gl, info = r0
    assert np.array_equal(gl, wl) and gl.dtype == np.int32 and same_bits(gv, wv) and np.array_equal(gf, m[1])
    assert info["rings_run"] == rings_run == 3 and info["n_layer_vertices"] == int((wl >= 1).sum()) > 0


mesh_case("locate_points", call_locate, check_locate, {"tube": tube})
mesh_case("split_rim_edges", call_split, check_split_case, OPEN_MESHES)
mesh_case("enforce_layer_gap", call_layers, check_layers, OPEN_MESHES)


# -- point kernels

def cloud(seed, n, centre=(10.0, -190.0, 1700.0)):
    return np.random.default_rng(seed).normal(0, 4, size=(n, 3)) + centre


def call_nn(e, t, request):
    return [mm.ccta.nn_min_sq(a, t[-1], engine=e) for a in t[:-1]]


def check_nn(e, t, r0, request):
    request.getfixturevalue("oracle")
    from oracle import oracle_ccta as occ
    occ.lib()
    for a, got in zip(t[:-1], r0):
        assert np.array_equal(got, occ.nn_min_sq(a, t[-1]))


point_case("nn_min_sq", call_nn, check_nn, lambda: tuple(cloud(n, n) for n in (255, 256, 257, 3001)) + (cloud(9, 700),))


def scene(nf):
    cc, ca, tris = _random_scene(nf * 7 + 16, nf, 17, 16)
    pts = np.concatenate([tris.reshape(-1, 3)[::5], np.random.default_rng(nf).uniform(-5, 20, (300, 3))])
    return cc, ca, tris, pts


def call_occluded(e, t, request):
    cc, ca, tris, pts = t
    return mm.ccta.occluded_point_flags(_cl(cc), _cl(ca), 1e9, pts, tris, 1.0, engine=e)


def check_occluded(e, t, r0, request):
    cc, ca, tris, pts = t
    want_rm, want_ex = LC.occluded(cc, ca, 1e9, pts, tris, 1.0)
    assert np.array_equal(r0[0].astype(bool), want_rm) and set(np.nonzero(r0[1])[0].tolist()) == want_ex and want_ex


def scene_twin(t):
    cc, ca, tris, pts = t
    return (twin_points(cc, 1, permute=False), twin_points(ca, 2, permute=False),
            twin_points(tris.reshape(-1, 3), 3).reshape(-1, 9), twin_points(pts, 4))


def scene_big(t):
    cc, ca, tris, pts = t
    return cc, ca, np.concatenate([tris, tris + 0.01, tris - 0.02]), big_points(pts)


for _nf in (257, 700):
    point_case(f"occluded_point_flags-{_nf}", call_occluded, check_occluded, lambda nf=_nf: scene(nf), scene_twin, scene_big)


def call_faces_near(e, m, request):
    return mm.find_faces_near_points(m[0], m[1], m[0][::3], engine=e)


def check_faces_near(e, m, r0, request):
    sel = LC.faces_near(m[0], m[1], m[0][::3])
    assert np.array_equal(r0, m[0][m[1][sel]]) and 0 < sel.sum()


mesh_case("find_faces_near_points", call_faces_near, check_faces_near)


def call_bounded(e, t, request):
    return [mm.find_centerline_bounded_points_simple(_cl(t[0]), p, 2.5, engine=e) for p in t[1:]]


def check_bounded(e, t, r0, request):
    for p, got in zip(t[1:], r0):
        want = p[LC.bounded(t[0], p, 2.5)]
        assert np.array_equal(got, want) and 0 < len(want) < len(p)


point_case("find_centerline_bounded_points_simple", call_bounded, check_bounded,
           lambda: (np.random.default_rng(6).uniform(-8, 8, (300, 3)),) +
           tuple(np.random.default_rng(n).uniform(-8, 8, (n, 3)) for n in (255, 256, 257, 3001)))


def branch_ids(m):
    b = np.arange(m) % 5
    return b


def call_masks(e, t, request):
    return [mm.branch_masks(make_cl(t[0], branch_ids(len(t[0]))), p, 1.5, engine=e) for p in t[1:]]


def check_masks(e, t, r0, request):
    for p, got in zip(t[1:], r0):
        want = CP.branch_masks(t[0], branch_ids(len(t[0])), p, 1.5)
        assert got.dtype == np.uint64 and np.array_equal(got, want) and want.any() and not want.all()


point_case("branch_masks", call_masks, check_masks,
           lambda: (np.random.default_rng(16).uniform(-10, 10, (700, 3)),) +
           tuple(np.random.default_rng(n + 1).uniform(-10, 10, (n, 3)) for n in (255, 256, 257, 3001)))


def vessel(seed):
    xyz, tan, bid, pts = curved_tube(seed)
    return xyz, tan, pts[0]


def contours_of(got):
    return [(c.id, c.original_frame, c.kind, np.asarray(c.centroid), np.asarray(c.points)) for c in got]


def call_vessel(e, t, request):
    xyz, tan, pts = t
    cl = Centerline.from_arrays(xyz, tan, branch_id=np.zeros(len(xyz), dtype=np.uint32))
    return contours_of(mm.discretize_vessel(cl, pts, 0, 1.0, 100, engine=e))


def check_vessel_case(e, t, r0, request):
    xyz, tan, pts = t
    got = check_vessel(e, xyz, tan, np.zeros(len(xyz), dtype=np.uint32), pts, 0, 1.0, 100)
    assert differences(contours_of(got), r0) == [] and len(got) > 5


def vessel_twin(t):
    xyz, tan, pts = vessel(13)                                            # another vessel of the same counts
    return xyz, tan, pts


def vessel_big(t):
    xyz, tan, bid, pts = curved_tube(14, n_cl=90, n_ring=30)
    return xyz, tan, pts[0]


point_case("discretize_vessel", call_vessel, check_vessel_case, lambda: vessel(12), vessel_twin, vessel_big)


def morph_jobs(seed):
    return [morph_case(seed + k, n_pts, n_cl) for k, (n_pts, n_cl) in enumerate([(255, 40), (256, 513), (257, 7), (3001, 600)])]


def call_morph(e, jobs, request):
    return mm.ccta.centerline_morph_batch([(cl_of(c), p, adj) for c, p, adj in jobs], e)


def check_morph(e, jobs, r0, request):
    request.getfixturevalue("oracle")
    from oracle import oracle_ccta as occ
    from oracle import oracle_cl as ocl
    occ.lib()
    ocl.lib()
    for (c, p, adj), (got, near) in zip(jobs, r0):
        want = occ.diameter_morphing(to_oracle_cl(ocl, cl_of(c)), p, adj)
        assert same_bits(got, want) and near.tolist() == SC.nearest_indices(c, p).tolist()


point_case("centerline_morph_batch", call_morph, check_morph, lambda: morph_jobs(50), lambda jobs: morph_jobs(70),
           lambda jobs: [morph_case(90 + k, 2 * len(p) + 11, 2 * len(c) + 3) for k, (c, p, _) in enumerate(jobs)])


def rings_of(seed):
    return [contour_ring(n, seed + k, centroid=bool(k % 2)) for k, n in enumerate((255, 256, 257, 3001))]


def call_measures(e, cs, request):
    got = mm.contour_measures(cs, engine=e)
    return {k: np.asarray(getattr(got, k)) for k in MEASURE_KEYS + MEASURE_PAIRS}


def check_measures(e, cs, r0, request):
    got = mm.contour_measures(cs, engine=e)
    assert_matches(cs, got)
    assert differences({k: np.asarray(getattr(got, k)) for k in MEASURE_KEYS + MEASURE_PAIRS}, r0) == []


point_case("contour_measures", call_measures, check_measures, lambda: rings_of(1), lambda cs: rings_of(31),
           lambda cs: [contour_ring(2 * n + 5, 61 + k) for k, n in enumerate((255, 256, 257, 3001))])


# -- the search engine: a transient plan (best_rotation_batch) and a resident one whose blobs come back from the blob cache
# (a plan of other contours of the same shapes was run and closed on the engine just before)

SEARCH_SIZES = ((255, 256), (257, 255), (256, 257), (521, 521))


def search_sets(seed):
    rng = np.random.default_rng(seed)
    return tuple(blob(rng, n) for pair in SEARCH_SIZES for n in pair)


def search_batch(sets):
    angles = mm.search_angles(1.0, 180.0)[0]
    n = len(sets) // 2
    return mm.Batch(list(sets[0::2]), list(sets[1::2]), [angles] * n, [(4.5, 4.5)] * n, [1] * n), angles


def call_transient(e, sets, request):
    batch, _ = search_batch(sets)
    return {prec: e.best_rotation_batch(batch, precision=prec, return_costs=True)
            for prec in (mm.MM_PRECISION_F64, mm.MM_PRECISION_F32)}


def call_resident(e, sets, request):
    batch, _ = search_batch(sets)
    out = {}
    for prec in (mm.MM_PRECISION_F64, mm.MM_PRECISION_F32):
        plan = e.plan(batch, prec)
        try:
            plan.run()
            out[prec] = plan.fetch(return_costs=True)
        finally:
            plan.close()
    return out


def check_search(e, sets, r0, request):
    oracle = request.getfixturevalue("oracle")
    batch, angles = search_batch(sets)
    for p in range(batch.n_pairs):
        oc = oracle.costs_over_angles(sets[2 * p], sets[2 * p + 1], angles, 4.5, 4.5, between=False)
        obi = int(np.argmin(oc))
        for prec, out in r0.items():
            assert out["best_idx"][p] == obi and out["best_angle"][p] == angles[obi] and out["best_cost"][p] == oc[obi]
        got = r0[mm.MM_PRECISION_F64]["costs"][batch.ang_off[p]:batch.ang_off[p + 1]]
        assert np.array_equal(got, oc)


for _name, _call in (("best_rotation_transient_plan", call_transient), ("best_rotation_resident_plan", call_resident)):
    point_case(_name, _call, check_search, lambda: search_sets(77),
               lambda sets: tuple(twin_points(s, 5 + k) for k, s in enumerate(sets)),
               lambda sets: tuple(blob(np.random.default_rng(200 + k), 2 * len(s) + 9) for k, s in enumerate(sets)))


# ---- the test ---------------------------------------------------------------------------------------------------------------

def test_the_ring_of_cases_names_every_entry_point_once():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names) > 40


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c.name for c in CASES])
def test_results_do_not_depend_on_what_the_buffers_held(engines, request, k):
    clean, dirty = engines
    case, other = CASES[k], CASES[(k + 1) % len(CASES)]
    x = case.x
    y, b = case.twin_of(x), case.big_of(x)
    r0 = case.call(clean, x, request)
    ry = case.call(dirty, y, request)                                     # the twin: every plane holds valid-looking words
    r1 = case.call(dirty, x, request)
    case.call(dirty, b, request)                                          # the buffers grow: X's planes inside B's leftovers
    r2 = case.call(dirty, x, request)
    other.call(dirty, other.x, request)                                   # another entry point carves them otherwise
    r3 = case.call(dirty, x, request)
    for name, r in (("behind the twin", r1), ("behind the larger input", r2), (f"behind {other.name}", r3)):
        assert differences(r0, r) == [], name
    case.check(clean, x, r0, request)
    assert differences(r0, ry) != [], "the twin gives the same result: the case shows nothing"
    assert uploads(r0) == uploads(ry)                                     # the same carving
    assert differences(r0, case.call(clean, x, request)) == []            # and the clean engine behind its own leftovers
