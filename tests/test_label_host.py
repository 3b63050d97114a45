"""CCTA mesh labelling, host side: the numpy checker (tests/mm_checkers/label_coronary.py) and the host C ABI
(mm_find_aortic_points, mm_final_reclassification) against known answers restated from the reference's own tests
(src/ccta/adjust_mesh/label_coronary.rs tests; tests/test_ccta.py TestFindAorticPoints / TestFindFacesNearPoints /
TestFinalReclassification), and against each other on random meshes.  No GPU."""
import numpy as np
import pytest

from mm_checkers import label_coronary as LC

import multimoda_rs_amd as mm


# ---- small meshes of the reference's tests, as data -----------------------------------------------------------------
GRID_V = [(float(x), float(y), 0.0) for y in range(3) for x in range(3)]          # 3 x 3 grid, vertex 4 in the centre
GRID_F = [[0, 1, 3], [1, 4, 3], [1, 2, 4], [2, 5, 4], [3, 4, 6], [4, 7, 6], [4, 5, 7], [5, 8, 7]]
ISLAND_V = [(float(i), 0.0, 0.0) for i in range(12)]                               # {0,1} next to {2..7}; {8..11} apart
ISLAND_F = [[0, 1, 2], [1, 4, 5], [0, 3, 4], [2, 3, 6], [4, 5, 7], [6, 7, 3], [8, 9, 10], [8, 10, 11]]
BLOB_V = [(float(i), 0.0, 0.0) for i in range(9)]                                  # removed 1, 2 around aorta 0; 7 = 8 apart
BLOB_F = [[1, 0, 2], [1, 3, 4], [2, 5, 6], [7, 8, 7]]
CHAIN_V = [(float(i), 0.0, 0.0) for i in range(6)]                                 # the path 0 - 1 - ... - 5
CHAIN_F = [[0, 1, 1], [1, 2, 2], [2, 3, 3], [3, 4, 4], [4, 5, 5]]
MESHES = {"grid": (GRID_V, GRID_F), "island": (ISLAND_V, ISLAND_F), "blob": (BLOB_V, BLOB_F), "chain": (CHAIN_V, CHAIN_F)}

# (mesh, rca, lca, rca_removed, lca_removed, {vertex: expected label}) -- 0 aorta, 1 rca, 2 lca, 3 / 4 removed
RECLASSIFY_CASES = {
    "isolated_rca_becomes_aorta": ("grid", [0, 6, 7, 8], [], [], [], {0: 0, 6: 1, 7: 1, 8: 1}),
    "isolated_lca_becomes_aorta": ("grid", [], [0, 6, 7, 8], [], [], {0: 0, 6: 2, 7: 2, 8: 2}),
    "non_isolated_rca_stays": ("grid", [0, 1], [], [], [], {0: 1, 1: 1}),
    "removed_rca_restored_by_rca_majority": ("grid", [1, 2, 3, 5, 6, 7], [], [4], [], {4: 1}),
    "aorta_island_promoted_to_rca": ("island", list(range(2, 8)), [], [], [], {0: 1, 1: 1}),
    "aorta_island_promoted_to_lca": ("island", [], list(range(2, 8)), [], [], {0: 2, 1: 2}),
    "aorta_island_stays_when_boundary_mixed": ("island", [2, 3], [4, 5], [], [], {0: 0, 1: 0}),
    "largest_component_never_reclassified": ("island", [0, 1, 8, 9, 10, 11], [], [], [], {i: 0 for i in range(2, 8)}),
    "restores_via_local_majority": ("blob", [3, 4, 5, 6], [], [1, 2], [], {1: 1, 2: 1}),
    "keeps_removed_when_local_majority_aorta": ("blob", [4, 6], [], [1, 2], [], {1: 3, 2: 3}),
    "keeps_fully_isolated_component_removed": ("blob", [], [], [7, 8], [], {7: 3, 8: 3}),
    "splits_chain_by_propagation": ("chain", [5], [], [1, 2, 3, 4], [], {1: 3, 2: 3, 3: 1, 4: 1}),
}


def _pts(v, idx):
    return np.asarray([v[i] for i in idx], dtype=np.float64).reshape(-1, 3)


def _native_labels(v, f, rca, lca, rr, lr):
    return mm.final_reclassification(v, f, rca, lca, rr, lr, return_labels=True)[5]


@pytest.mark.parametrize("name", sorted(RECLASSIFY_CASES))
def test_final_reclassification_known_answers(name):
    mesh, rca, lca, rr, lr, want = RECLASSIFY_CASES[name]
    v, f = MESHES[mesh]
    args = [_pts(v, rca), _pts(v, lca), _pts(v, rr), _pts(v, lr)]
    lab_checker = LC.reclassify(v, f, *args)
    lab_native = _native_labels(v, f, *args)
    for i, l in want.items():
        assert lab_checker[i] == l, (name, i, lab_checker)
    assert np.array_equal(lab_native, lab_checker), (name, lab_native, lab_checker)


def test_final_reclassification_outputs_partition_the_vertices():
    v, f = MESHES["grid"]
    out = mm.final_reclassification(v, f, _pts(v, [0, 1]), _pts(v, [2, 3]), _pts(v, []), _pts(v, []))
    assert sum(a.shape[0] for a in out) == len(v)
    assert all(a.shape[1:] == (3,) for a in out)
    assert np.array_equal(np.sort(np.concatenate(out), axis=0), np.sort(np.asarray(v), axis=0))


def test_largest_component_tie_keeps_the_smallest_vertex_index():
    # path 0 - 1 - ... - 6; RCA components {0, 1} and {5, 6} are equally large: {0, 1} stays, {5, 6} (boundary: the
    # aortic vertex 4 only) joins the aorta -- one of the outcomes the reference's hash order can produce
    v = [(float(i), 0.0, 0.0) for i in range(7)]
    f = [[i, i + 1, i + 1] for i in range(6)]
    want = [1, 1, 0, 0, 0, 0, 0]
    args = [_pts(v, [0, 1, 5, 6]), _pts(v, []), _pts(v, []), _pts(v, [])]
    assert LC.reclassify(v, f, *args).tolist() == want
    assert _native_labels(v, f, *args).tolist() == want


def test_duplicate_coordinates_label_the_last_vertex():
    # vertex 9 repeats the centre vertex 4 and belongs to no face: the removed label lands on 9 (the last index), not 4
    v = GRID_V + [GRID_V[4]]
    f = GRID_F
    args = [_pts(v, [1, 2, 3, 5, 6, 7]), _pts(v, []), _pts(v, [4]), _pts(v, [])]
    lab = _native_labels(v, f, *args)
    assert np.array_equal(lab, LC.reclassify(v, f, *args))
    assert lab[9] == 3 and lab[4] == 1 and lab[0] == 0 and lab[8] == 1
    # both copies leave the aortic set
    kept = mm.find_aortic_points(v, _pts(v, [4]), _pts(v, []))
    assert kept.shape[0] == len(v) - 2


def test_face_index_out_of_range_is_an_error():
    v, f = MESHES["grid"]
    with pytest.raises(RuntimeError):
        mm.final_reclassification(v, f + [[0, 1, 9]], _pts(v, [0]), _pts(v, []), _pts(v, []), _pts(v, []))
    with pytest.raises(RuntimeError):
        mm.final_reclassification(v, [[0, -1, 2]], _pts(v, [0]), _pts(v, []), _pts(v, []), _pts(v, []))


# ---- find_aortic_points ---------------------------------------------------------------------------------------------
def test_find_aortic_points_known_answers():
    v = GRID_V[:2] + [GRID_V[3], GRID_V[4]]
    got = mm.find_aortic_points(v, [v[0]], [v[1]])
    assert got.tolist() == [list(v[2]), list(v[3])]
    assert mm.find_aortic_points(v, [], []).shape == (4, 3)
    g = mm.find_aortic_points(GRID_V, GRID_V[:5], GRID_V[5:])
    assert g.shape == (0, 3)
    g = mm.find_aortic_points(GRID_V, [GRID_V[0]], [GRID_V[1]])
    assert g.tolist() == [list(p) for p in GRID_V[2:]]
    assert np.array_equal(LC.aortic_mask(GRID_V, [GRID_V[0]], [GRID_V[1]]), [False, False] + [True] * 7)


def test_find_aortic_points_is_bit_exact():
    v = [(0.0, 0.0, 0.0), (-0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (np.nextafter(1.0, 2.0), 1.0, 1.0)]
    got = mm.find_aortic_points(v, [(0.0, 0.0, 0.0)], [(1.0, 1.0, 1.0)])
    assert got.shape == (2, 3)
    assert np.signbit(got[0, 0]) and got[1, 0] == np.nextafter(1.0, 2.0)
    assert np.array_equal(LC.aortic_mask(v, [(0.0, 0.0, 0.0)], [(1.0, 1.0, 1.0)]), [False, True, False, True])


# ---- checker known answers of the device functions (the GPU tests compare the device against the checker) ---------
def test_checker_single_ray_triangle():
    ok, t = LC.ray_hits(np.zeros(3), np.array([1.0, 0.0, 0.0]), [[1.0, -1.0, -1.0, 1.0, 1.0, -1.0, 1.0, 0.0, 1.0]])
    assert ok[0] and abs(t[0] - 1.0) < 1e-6


def test_checker_bounded_points_simple_geometry():
    inside = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.5, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 1.0), (0.5, 1.0, 1.0),
              (0.0, 0.0, 2.0), (1.0, 0.0, 2.0), (0.5, 1.0, 2.0)]
    outside = [(-1.0, -1.0, z) for z in (0.5, 1.5, 2.5)] + [(2.0, -1.0, z) for z in (0.5, 1.5, 2.5)] + \
              [(0.5, 2.0, z) for z in (0.5, 1.5, 2.5)]
    cl = [(0.5, 0.5, 0.0), (0.5, 0.5, 1.0), (0.5, 0.5, 2.0)]
    m = LC.bounded(cl, inside + outside, 1.0)
    assert m.tolist() == [True] * 9 + [False] * 9


def test_checker_faces_near_points_known_answers():
    v4 = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)]
    f4 = [[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]]
    assert LC.faces_near(v4, f4, [(0.0, 0.0, 0.0)]).tolist() == [True, True, True, False]
    assert not LC.faces_near(v4[:3], [[0, 1, 2]], [(5.0, 5.0, 5.0)]).any()
    assert LC.faces_near(GRID_V, GRID_F, [(0.0, 0.0, 0.0)]).tolist() == [True] + [False] * 7
    assert LC.faces_near(GRID_V, GRID_F, [(1.0, 1.0, 0.0)]).sum() == 6
    assert not LC.faces_near(GRID_V, GRID_F, np.zeros((0, 3))).any()
    assert not LC.faces_near(GRID_V, GRID_F, [(99.0, 99.0, 0.0)]).any()


def test_checker_ray_list_follows_take_and_step_by():
    cc = [(0.0, 0.0, float(z)) for z in range(10)]          # spacing 1
    ca = [(5.0, 0.0, 0.0), (5.0, 0.0, 1.0)]                  # spacing 1
    o, d = LC.ray_list(cc, ca, 6.5, 2.0)                     # take(7).step_by(2): 0, 2, 4, 6
    assert o.shape == (8, 3)
    assert np.array_equal(d[:4] + o[:4], np.asarray(cc)[[0, 2, 4, 6]])
    assert LC.ray_list(cc, ca, 6.5, 0.0) is None             # step 0: the reference panics
    assert LC.ray_list(cc, ca, float("nan"), 1.0)[0].shape == (0, 3)
    assert LC.ray_list(cc, ca, float("inf"), 1.0)[0].shape == (20, 3)


# ---- random meshes: checker and host ABI agree ----------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_final_reclassification_random_meshes(seed):
    rng = np.random.default_rng(seed)
    nv = int(rng.integers(5, 80))
    v = rng.integers(0, 6, size=(nv, 3)).astype(np.float64)     # small integer grid: duplicated coordinates happen
    f = rng.integers(0, nv, size=(int(rng.integers(1, 3 * nv)), 3))
    perm = rng.permutation(nv)
    cuts = np.sort(rng.integers(0, nv + 1, size=4))
    parts = [v[perm[a:b]] for a, b in zip([0] + cuts.tolist(), cuts.tolist())]
    parts = [np.concatenate([p, p[: int(rng.integers(0, 2))]]) for p in parts]   # a repeated point now and then
    lab = _native_labels(v, f, *parts)
    assert np.array_equal(lab, LC.reclassify(v, f, *parts)), seed
    keep = mm.find_aortic_points(v, parts[0], parts[1])
    assert np.array_equal(keep, v[LC.aortic_mask(v, parts[0], parts[1])])
