"""CCTA mesh trimming on the device (csrc/mm_trim_kernels.hip) against the checker (tests/mm_checkers/trim_mesh.py):
identical indices and bit-identical coordinates on grids, random meshes with degenerate and repeated faces and
duplicated coordinates, -0.0 / NaN vertices, empty and no-match inputs, a table that needs probing and a mesh of more
than 10^6 faces; and the pipeline label_geometry -> label_anomalous_region -> remove -> morph + sync -> keep / export
on the synthetic acute take-off mesh."""
import numpy as np
import pytest

from mm_checkers import trim_mesh as TM
from test_trim_host import grid_with_hole, full_grid, octahedron, capped_tube, traces_real_edges
from test_trim_host import CARRY_NV, band_across_the_carry

import multimoda_rs_amd as mm

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_points(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 3), np.asarray(b, dtype=np.float64).reshape(-1, 3)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def same_results(got, want):
    assert sorted(got) == sorted(want)
    gv, gf = got["mesh"]
    wv, wf = want["mesh"]
    assert same_points(gv, wv) and np.array_equal(np.asarray(gf), np.asarray(wf))
    for k in want:
        if k != "mesh":
            assert same_points(got[k], want[k]), k


def cl_of(xyz):
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    a = np.zeros(xyz.shape[0], dtype=mm.centerline.CL_DTYPE)
    a["x"], a["y"], a["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return mm.Centerline(a)


def random_mesh(seed, nv=400, nf=1500):
    """Faces on a random surface-like index pattern, with degenerate faces, repeated faces and duplicated coordinates."""
    r = np.random.default_rng(seed)
    v = np.round(r.normal(size=(nv, 3)), 1)
    v[r.integers(0, nv, 20)] = v[r.integers(0, nv, 20)]                          # duplicated coordinates
    base = r.integers(0, nv - 2, nf)
    f = np.stack([base, base + 1, base + r.integers(1, 3, nf)], 1)
    f[:30, 1] = f[:30, 0]                                                          # degenerate faces
    f = np.concatenate([f, f[40:70]])                                              # repeated faces
    return v, f.astype(np.int64)


# ---- open edges, rings ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["grid", "pinch", "octahedron", "tube", "random0", "random1"])
def test_open_edges_and_rings_equal_the_checker(engine, case):
    if case == "grid":
        v, f, _, seeds = grid_with_hole()
    elif case == "pinch":
        v, f, _, seeds = grid_with_hole(remove=[(4, 4), (6, 6)])
    elif case == "octahedron":
        (v, f), seeds = octahedron(), {1}
    elif case == "tube":
        (v, f), seeds = capped_tube(), {0}
    else:
        v, f = random_mesh(int(case[-1]))
        seeds = set(range(0, 400, 7))
    assert np.array_equal(mm.open_boundary_edges(f, engine=engine), TM.open_boundary_edges(f))
    for s in (seeds, None):
        for t in (None, 1, 2):
            got = mm.order_boundary_rings(f, v, s, t, engine=engine)
            assert [r.tolist() for r in got] == TM.order_boundary_rings(f, v, s, t)
    for s in (seeds, set(), {10_000}):
        for t, rounds in ((1, 64), (2, 64), (1, 1), (1, 0)):
            drop, rings = mm.clean_open_boundary(f, v, s, t, max_rounds=rounds, engine=engine)
            wd, wr = TM.clean_open_boundary(f, v, s, t, max_rounds=rounds)
            assert drop.tolist() == wd and [r.tolist() for r in rings] == wr


def test_pinch_cull_on_the_device(engine):
    v, f, _, seeds = grid_with_hole(remove=[(4, 4), (6, 6)])
    drop, rings = mm.clean_open_boundary(f, v, seeds, engine=engine)
    assert len(drop) == 1
    surviving = f[~np.any(np.isin(f, drop), axis=1)]
    assert traces_real_edges(surviving, rings[0])


def test_a_table_that_needs_probing(engine):
    """Many distinct edges (most of them open) in one table: collisions and long probe runs."""
    r = np.random.default_rng(11)
    f = r.integers(0, 60_000, size=(200_000, 3)).astype(np.int64)
    f = np.concatenate([f, f[:50_000]])
    assert np.array_equal(mm.open_boundary_edges(f, engine=engine), TM.open_boundary_edges(f))


def test_degenerate_edges_count(engine):
    f = np.array([[0, 0, 1], [0, 1, 2], [2, 2, 2]])
    assert mm.open_boundary_edges(f, engine=engine).tolist() == TM.open_boundary_edges(f).tolist()


# ---- remove / keep / border faces ----------------------------------------------------------------------------------

def labelled(v, f, seed):
    r = np.random.default_rng(seed)
    lab = r.integers(0, 4, v.shape[0])
    res = {"mesh": (v, f), "aorta_points": v[lab == 0], "rca_points": v[lab == 1], "lca_points": v[lab == 2],
           "anomalous_points": v[(lab == 3)][: 40], "distal_points": v[::9], "boundary_points_4": v[:2],
           "extra": np.array([[1.0, 2.0, 3.0]])}
    return res


@pytest.mark.parametrize("seed", range(4))
def test_remove_keep_extract_on_random_meshes(engine, seed):
    v, f = random_mesh(seed)
    for key, tb in (("anomalous_points", 1), (["lca_points", "anomalous_points"], 2), ("rca_points", 3)):
        same_results(mm.remove_labeled_points_from_mesh(labelled(v, f, seed), key, tb, engine=engine),
                     TM.remove_labeled_points_from_mesh(labelled(v, f, seed), key, tb))
        same_results(mm.keep_labeled_points_from_mesh(labelled(v, f, seed), key, tb, engine=engine),
                     TM.keep_labeled_points_from_mesh(labelled(v, f, seed), key, tb))
    res = labelled(v, f, seed)
    gv, gf = mm.extract_region_with_border_faces((v, f), res["rca_points"], engine=engine)
    wv, wf = TM.extract_region_with_border_faces((v, f), res["rca_points"])
    assert same_points(gv, wv) and np.array_equal(gf, wf)


def test_grid_remove_gives_the_hole_ring(engine):
    v, f = full_grid()
    t = v[[39, 40, 41, 49]]
    res = {"mesh": (v, f), "anomalous_points": t, "rca_points": v[:27]}
    got = mm.remove_labeled_points_from_mesh(res, "anomalous_points", engine=engine)
    same_results(got, TM.remove_labeled_points_from_mesh(dict(res), "anomalous_points"))
    assert got["anomalous_points"].shape == (0, 3) and len(got["boundary_points_1"]) > 0
    assert "boundary_points_2" not in got
    res_list = mm.remove_labeled_points_from_mesh(dict(res), ["anomalous_points"], engine=engine)
    same_results(res_list, got)


def test_signed_zero_and_nan_vertices(engine):
    v, f = full_grid(6)
    v = v - 2.0
    v[14] = [0.0, -0.0, 0.0]
    v[20] = [np.nan, 1.0, 0.0]
    res = {"mesh": (v, f), "anomalous_points": np.array([[-0.0, 0.0, -0.0], [np.nan, 1.0, 0.0], v[15], v[21]]),
           "rca_points": v[:12], "lca_points": np.array([[np.nan, 1.0, 0.0]])}
    got = mm.remove_labeled_points_from_mesh(dict(res), "anomalous_points", engine=engine)
    want = TM.remove_labeled_points_from_mesh(dict(res), "anomalous_points")
    assert len(got["mesh"][0]) == 36 - 3                                            # NaN row matches nothing
    assert np.isnan(got["mesh"][0]).any()
    gv, wv = got["mesh"][0], want["mesh"][0]
    assert np.array_equal(bits(gv), bits(wv)) and np.array_equal(got["mesh"][1], want["mesh"][1])
    assert got["lca_points"].shape == (0, 3)
    for k in ("rca_points", "boundary_points", "boundary_points_1"):
        assert same_points(got[k], want[k]), k


def test_empty_and_no_match(engine):
    v, f = full_grid(4)
    res = {"mesh": (v, f), "anomalous_points": np.zeros((0, 3)), "rca_points": np.array([[50.0, 50.0, 50.0]])}
    assert mm.remove_labeled_points_from_mesh(res, engine=engine) is res
    assert mm.remove_labeled_points_from_mesh(res, "rca_points", engine=engine) is res
    assert mm.keep_labeled_points_from_mesh(res, ["rca_points", "missing"], engine=engine) is res
    ev, ef = mm.extract_region_with_border_faces((v, f), [[50.0, 50.0, 50.0]], engine=engine)
    assert ev.shape == (0, 3) and ef.shape == (0, 3)
    assert mm.open_boundary_edges(np.zeros((0, 3), dtype=np.int64), engine=engine).shape == (0, 2)
    assert mm.order_boundary_rings(np.zeros((0, 3)), v, engine=engine) == []
    drop, rings = mm.clean_open_boundary(np.zeros((0, 3)), v, {1}, engine=engine)
    assert drop.size == 0 and rings == []
    # the whole mesh kept: no seeds, so every rim is cleaned (the reference's empty-seed rule)
    out = mm.keep_labeled_points_from_mesh({"mesh": (v, f), "rca_points": v}, "rca_points", engine=engine)
    same_results(out, TM.keep_labeled_points_from_mesh({"mesh": (v, f), "rca_points": v}, "rca_points"))


def test_a_million_faces(engine):
    v, f, *_ = mm.synth.synthetic_takeoff_mesh(n_theta=1024, n_z=500)
    assert f.shape[0] >= 10 ** 6
    band = (v[:, 2] > 20.0) & (v[:, 2] < 26.0) & (v[:, 0] > 0.0)
    res = {"mesh": (v, f), "anomalous_points": v[band], "aorta_points": v[~band][::3]}
    got = mm.remove_labeled_points_from_mesh(dict(res), "anomalous_points", engine=engine)
    same_results(got, TM.remove_labeled_points_from_mesh(dict(res), "anomalous_points"))
    assert len(got["boundary_points_1"]) > 0
    assert np.array_equal(mm.open_boundary_edges(f, engine=engine), TM.open_boundary_edges(f))


def test_more_tiles_than_one_round_of_the_tile_scan(engine):
    """258 tiles of vertices: the one-workgroup scan of the tile counts (256 a round) carries into a second round.  The
    band's faces hold 0, 4095, 4096, 2^20 - 1, 2^20 and nv - 1; the region takes a band vertex and isolated vertices on
    each side of 2^20, so the kept vertices beyond it get their new index from the carry."""
    v, f, lower, _ = band_across_the_carry()
    nv = len(v)
    assert nv == CARRY_NV and {0, 4095, 4096, 2 ** 20 - 1, 2 ** 20, nv - 1} <= set(f.ravel().tolist())
    region = np.concatenate([lower[[10, 90]], np.arange(5000, 6000), np.arange(2 ** 20 + 1000, 2 ** 20 + 1100)])
    assert (region < 2 ** 20).sum() == 1002 and (region > 2 ** 20).sum() == 100
    res = {"mesh": (v, f), "anomalous_points": v[region]}
    got = mm.remove_labeled_points_from_mesh(dict(res), "anomalous_points", engine=engine)
    want = TM.remove_labeled_points_from_mesh(dict(res), "anomalous_points")
    same_results(got, want)
    gv, gf = got["mesh"]
    assert len(gv) <= nv - len(region) and len(gv) > 2 ** 20 and len(gf) > 0
    assert gf.min() < 4096 and gf.max() == len(gv) - 1 and same_points(gv[-1], v[-1])
    assert len(got["boundary_points_1"]) > 0


# ---- pipeline ----------------------------------------------------------------------------------------------------------

def test_pipeline_on_the_takeoff_mesh(engine, tmp_path):
    v, f, ca, cr, cll, _ = mm.synth.synthetic_takeoff_mesh()
    cla, clr, cl_l = cl_of(ca), cl_of(cr), cl_of(cll)
    res = mm.label_geometry((v, f), cla, clr, cl_l, acute_takeoff_rca=True, engine=engine)
    res = mm.label_anomalous_region(clr, cr[20:52:2], res, engine=engine)
    anomalous = np.asarray(res["anomalous_points"])
    assert len(anomalous) > 0
    want = TM.remove_labeled_points_from_mesh(dict(res), "anomalous_points", target_boundaries=2)
    got = mm.remove_labeled_points_from_mesh(dict(res), "anomalous_points", target_boundaries=2, engine=engine)
    same_results(got, want)
    near = lambda p: np.argmin(((p[:, None, :] - cr[None]) ** 2).sum(-1), axis=1)     # noqa: E731
    lo, hi = near(anomalous).min(), near(anomalous).max()
    # the occluded side of the section is labelled rca_removed / aorta, so the cut leaves one rim around the strip that
    # joins the proximal and distal stumps; it runs from one end of the section to the other
    assert [k for k in got if k.startswith("boundary_points_")] == ["boundary_points_1"]
    idx = mm.ccta._match(got["mesh"][0], got["boundary_points_1"])
    assert (idx >= 0).all() and traces_real_edges(got["mesh"][1], idx.tolist())
    reach = near(got["boundary_points_1"])
    assert reach.min() <= lo and reach.max() >= hi

    # a cut through the whole section (every tube vertex of its rings) leaves two rings, one at each end
    n_around = 16
    na = v.shape[0] - 2 * len(cr) * n_around
    ring_of = (np.arange(v.shape[0]) - na) // n_around
    in_tube = (np.arange(v.shape[0]) >= na) & (np.arange(v.shape[0]) < na + len(cr) * n_around)
    rings_hit = ring_of[mm.ccta._match(v, anomalous)]
    section = in_tube & (ring_of >= rings_hit.min()) & (ring_of <= rings_hit.max())
    res["section_points"] = v[section]
    want = TM.remove_labeled_points_from_mesh(dict(res), "section_points", target_boundaries=2)
    got = mm.remove_labeled_points_from_mesh(dict(res), "section_points", target_boundaries=2, engine=engine)
    same_results(got, want)
    nv_, nf_ = got["mesh"]
    assert "boundary_points_1" in got and "boundary_points_2" in got and "boundary_points_3" not in got
    for k in ("boundary_points_1", "boundary_points_2"):                 # closed walks along real open edges
        idx = mm.ccta._match(nv_, got[k])
        assert (idx >= 0).all() and traces_real_edges(nf_, idx.tolist()), k
    ends = sorted(float(np.mean(near(got[k]))) for k in ("boundary_points_1", "boundary_points_2"))
    assert abs(ends[0] - lo) < abs(ends[0] - hi) and abs(ends[1] - hi) < abs(ends[1] - lo)

    # a morph + sync round keeps the rings on the moved vertices
    m = mm.scale_region_centerline_morphing(got["mesh"], got["distal_points"], clr, -0.2, engine=engine)
    synced = mm.sync_results_to_mesh(got, got["mesh"], m)
    for k in ("boundary_points_1", "boundary_points_2"):
        idx = mm.ccta._match(nv_, got[k])
        assert np.array_equal(bits(synced[k]), bits(m[0][idx])), k

    # keep the aorta with its removed regions, export every section
    del res["section_points"]
    keys = ["aorta_points", "rca_removed_points", "lca_removed_points"]
    same_results(mm.keep_labeled_points_from_mesh(dict(res), keys, engine=engine),
                 TM.keep_labeled_points_from_mesh(dict(res), keys))
    for typ in ("all", "aorta", "rca", "lca"):
        path = mm.export_section_stl(res, typ, tmp_path, engine=engine)
        _, tri = TM.read_stl(path)
        sv, sf = TM.section_mesh(res, typ)
        assert len(sf) > 0 and np.array_equal(tri, np.asarray(sv)[np.asarray(sf)].astype(np.float32)), typ
