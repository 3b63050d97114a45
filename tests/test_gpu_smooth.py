"""CCTA mesh finishing on the device (csrc/mm_smooth_kernels.hip, csrc/mm_smooth.cpp) against the checker
(tests/mm_checkers/smooth_mesh.py): the identical CSR (offsets, neighbours, info), bit-identical coordinates, volumes and
largest displacement, equal integer report fields and the launch count include/mm_ccta.h states.  Shapes: the small
solids, tubes whose cap centre has a row longer than a wave (70) and than a workgroup (300), meshes one vertex past a
workgroup (257) and past a scan tile (4097), a messy face list, shuffled faces, step counts 0 / 1 / 11, arbitrary
factors, pins, bands, random meshes, the errors, and the line label -> remove -> stitch(fill_holes=True, smooth=True)."""
import ctypes as C
import os

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings, strategies as st

from mm_checkers import close_mesh as CM
from mm_checkers import smooth_mesh as SMO
from mm_checkers import stitch_mesh as SM
from test_trim_host import octahedron, capped_tube, CARRY_NV, band_across_the_carry
from test_close_host import open_box
from test_smooth_host import tetrahedron, noisy_icosphere, same_bits
from test_gpu_stitch import takeoff_case

import multimoda_rs_amd as mm
from multimoda_rs_amd import ccta

pytestmark = pytest.mark.gpu

INT_KEYS = ("n_vertices", "n_faces", "n_edges", "n_isolated", "n_pinned", "max_degree", "steps_run", "launches")
TAUBIN10 = SMO.taubin_factors(0.5, 0.5, 10)


def bits_equal(a, b):
    return np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


def same_csr(f, nv, engine):
    off, nb, info = mm.mesh_adjacency_csr(f, nv, engine=engine)
    woff, wnb, winfo = SMO.csr(f, nv)
    assert off.dtype == np.int64 and np.array_equal(off, woff) and np.array_equal(nb, wnb)
    assert info == {"entries": winfo["entries"], "max_degree": winfo["max_degree"], "n_isolated": winfo["isolated"],
                    "launches": winfo["launches"]}
    return off, nb, info


def same_smooth(v, f, factors, engine, pinned=None):
    got, rep = mm.smooth_mesh((v, f), factors, pinned=pinned, engine=engine)
    want, wrep = SMO.smooth(v, f, factors, pinned)
    assert got[1] is f and same_bits(got[0], want)
    for k in INT_KEYS:
        assert rep[k] == wrep[k], (k, rep[k], wrep[k])
    for k in ("volume_before", "volume_after", "max_displacement_sq"):
        assert bits_equal(rep[k], wrep[k]), (k, rep[k], wrep[k])
    return got[0], rep


def jitter(v, seed):
    return v + 0.05 * np.random.default_rng(seed).standard_normal(v.shape)


# ---- shapes ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("solid", [tetrahedron, octahedron, open_box])
def test_small_solids(engine, solid):
    v, f = solid()
    same_csr(f, len(v), engine)
    out, rep = same_smooth(v, f, TAUBIN10, engine)
    if solid is octahedron:
        assert same_bits(out, v * 0.2373046875) and rep["launches"] == 7 + 10 + 2 * 2 + 1
    same_smooth(jitter(v, 1), f, [0.5] * 3, engine)


@pytest.mark.parametrize("n_around,n_rings", [(70, 3), (300, 3)])
def test_cap_centre_row_longer_than_a_wave_and_a_workgroup(engine, n_around, n_rings):
    v, f = capped_tube(n_around, n_rings)
    v = jitter(v, n_around)
    off, nb, info = same_csr(f, len(v), engine)
    assert info["max_degree"] == n_around and off[-1] - off[-2] == n_around
    _, rep = same_smooth(v, f, TAUBIN10, engine)
    assert rep["max_degree"] == n_around


@pytest.mark.parametrize("n_around,n_rings", [(15, 17), (63, 65)])
def test_one_vertex_past_a_workgroup_and_past_a_scan_tile(engine, n_around, n_rings):
    v, f = capped_tube(n_around, n_rings)
    assert len(v) in (257, 4097)
    v = jitter(v, n_rings)
    same_csr(f, len(v), engine)
    same_smooth(v, f, TAUBIN10, engine)
    ring, info = ccta.vertex_rings_info(f, [len(v) - 2], 10 ** 6, len(v), engine=engine)
    wring, winfo = SMO.rings(f, len(v), [len(v) - 2], 10 ** 6)
    assert np.array_equal(ring, wring) and info == winfo and info["reached"] == len(v)


def test_more_tiles_than_one_round_of_the_tile_scan(engine):
    """258 tiles of degrees: the one-workgroup scan of the tile sums (256 a round) carries into a second round, and the
    rows beyond vertex 2^20 start at offsets that come from the carry."""
    _, f, _, _ = band_across_the_carry()
    off, nb, info = same_csr(f, CARRY_NV, engine)
    assert off[2 ** 20 + 1] > 0 and off[2 ** 20 + 1] < off[-1] == len(nb)
    assert info["n_isolated"] == CARRY_NV - 300 and info["max_degree"] == 4


def messy():
    """Two bodies (a jittered tube and an octahedron), repeated faces, (a, a, b) faces and two isolated vertices."""
    tv, tf = capped_tube(9, 4)
    ov, of = octahedron()
    v = np.concatenate([jitter(tv, 3), ov + [5.0, 0, 0], [[9.0, 9.0, 9.0], [-0.0, 1.0, 2.0]]])
    n = len(tv)
    f = np.concatenate([tf, of + n, tf[:7], of[:2] + n, [[0, 0, 1], [3, 4, 3], [n, n + 1, n + 1], [2, 2, 2]]])
    return v, f


def test_messy_face_list_two_bodies_isolated_vertices(engine):
    v, f = messy()
    _, _, info = same_csr(f, len(v), engine)
    assert info["n_isolated"] == 2
    out, rep = same_smooth(v, f, TAUBIN10, engine)
    assert rep["n_isolated"] == 2 and same_bits(out[-2:], v[-2:])
    # vertices beyond the largest index, and no face at all
    same_csr(f, len(v) + 5, engine)
    empty = np.zeros((0, 3), dtype=np.int64)
    off, nb, info = same_csr(empty, 3, engine)
    assert off.tolist() == [0, 0, 0, 0] and info["launches"] == 0
    out, rep = same_smooth(v[:3], empty, TAUBIN10, engine)
    assert same_bits(out, v[:3]) and rep["launches"] == 0 and rep["n_isolated"] == 3


def test_shuffled_faces_give_the_same_bits(engine):
    v, f = noisy_icosphere()
    off, nb, _ = same_csr(f, len(v), engine)
    out, rep = same_smooth(v, f, TAUBIN10, engine)
    r = np.random.default_rng(5)
    for _ in range(3):
        g = f[r.permutation(len(f))]
        g = np.stack([np.roll(t, int(k)) for t, k in zip(g, r.integers(0, 3, len(g)))])
        off2, nb2, _ = mm.mesh_adjacency_csr(g, len(v), engine=engine)
        assert np.array_equal(off2, off) and np.array_equal(nb2, nb)
        got, _ = mm.smooth_mesh((v, g), TAUBIN10, engine=engine)
        assert same_bits(got[0], out)                                   # the volume's tree follows the face order; the vertices do not


@pytest.mark.parametrize("n_steps", [0, 1, 2, 11])
def test_step_counts(engine, n_steps):
    v, f = noisy_icosphere()
    factors = SMO.taubin_factors(0.5, 0.5, n_steps)
    out, rep = same_smooth(v, f, factors, engine)
    assert rep["steps_run"] == n_steps and rep["launches"] == 7 + n_steps + 2 * SMO.volume_launches(len(f)) + 1
    if n_steps == 0:
        assert same_bits(out, v) and bits_equal(rep["volume_before"], rep["volume_after"]) and rep["max_displacement_sq"] == 0.0
    else:
        assert factors[-1] == (0.5 if n_steps % 2 else -0.5)
    via = mm.filter_taubin((v, f), 0.5, 0.5, n_steps, engine=engine)
    assert same_bits(via[0], out)
    lap = mm.filter_laplacian((v, f), 0.3, n_steps, engine=engine)
    assert same_bits(lap[0], SMO.smooth(v, f, [0.3] * n_steps)[0])


def test_arbitrary_factors(engine):
    v, f = noisy_icosphere()
    same_smooth(v, f, [0.7, -0.31, 0.0, 1.0, -1.5, 0.123456789], engine)


def test_pinned_every_third_vertex(engine):
    v, f = noisy_icosphere()
    mask = np.arange(len(v)) % 3 == 0
    out, rep = same_smooth(v, f, TAUBIN10, engine, pinned=mask)
    assert rep["n_pinned"] == int(mask.sum()) and same_bits(out[mask], v[mask])
    assert not (out[~mask] == v[~mask]).all(axis=1).any()
    by_index, _ = mm.smooth_mesh((v, f), TAUBIN10, pinned=np.flatnonzero(mask), engine=engine)
    assert same_bits(by_index[0], out)

    class Mesh:
        def __init__(self, vertices, faces):
            self.vertices, self.faces = vertices, faces

    src = Mesh(v.copy(), f)
    m, _ = mm.smooth_mesh(src, TAUBIN10, pinned=mask, engine=engine)
    assert isinstance(m, Mesh) and m is not src and same_bits(m.vertices, out) and same_bits(src.vertices, v)
    post = mm.postprocess_stitched_mesh((v, f), postprocessing=True, pinned=mask, engine=engine)
    assert same_bits(post[0], out)


def test_band_equals_a_hand_built_mask(engine):
    v, f = capped_tube(12, 20)
    v = jitter(v, 7)
    seeds = np.arange(5 * 12, 6 * 12)                                   # one ring of the tube
    ring = mm.vertex_rings(f, seeds, 3, len(v), engine=engine)
    wring, _ = SMO.rings(f, len(v), seeds, 3)
    assert ring.dtype == np.int32 and np.array_equal(ring, wring)
    hand = np.ones(len(v), dtype=bool)
    hand[2 * 12: 9 * 12] = False                                        # the rings 2 .. 8 of the tube: within 3 edges
    assert np.array_equal(ring < 0, hand)
    band, rep = mm.smooth_mesh((v, f), TAUBIN10, band=(seeds, 3), engine=engine)
    want, wrep = SMO.smooth(v, f, TAUBIN10, hand)
    assert same_bits(band[0], want) and rep["n_pinned"] == int(hand.sum()) == wrep["n_pinned"]
    by_xyz, _ = mm.smooth_mesh((v, f), TAUBIN10, band=(v[seeds], 3), engine=engine)
    assert same_bits(by_xyz[0], want)
    extra = np.zeros(len(v), dtype=bool)
    extra[5 * 12] = True                                                # OR-ed with a pin inside the band
    both, _ = mm.smooth_mesh((v, f), TAUBIN10, band=(seeds, 3), pinned=extra, engine=engine)
    assert same_bits(both[0], SMO.smooth(v, f, TAUBIN10, hand | extra)[0])
    # cut-off, an unreachable body, a repeated seed
    v2, f2 = messy()
    for max_ring in (0, 1, 2, 50):
        got, info = ccta.vertex_rings_info(f2, [0, 0, 4], max_ring, len(v2), engine=engine)
        wgot, winfo = SMO.rings(f2, len(v2), [0, 0, 4], max_ring)
        assert np.array_equal(got, wgot) and info == winfo
    assert (got[len(capped_tube(9, 4)[0]):] == -1).all()


@settings(max_examples=40 * int(os.environ.get("MM_HYP_SCALE", "1")), deadline=None, derandomize=True, database=None,
          suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(seed=st.integers(0, 2**31 - 1), nv=st.integers(1, 70), nf=st.integers(0, 160), n_steps=st.integers(0, 5),
       pin=st.sampled_from([None, 0.0, 0.3, 1.0]))
def test_random_small_meshes_and_masks(engine, seed, nv, nf, n_steps, pin):
    r = np.random.default_rng(seed)
    v = r.uniform(-3, 3, (nv, 3))
    f = r.integers(0, nv, (nf, 3))
    factors = r.choice([0.5, -0.5, 0.25, -0.53, 0.0, 1.0], n_steps).tolist()
    pinned = None if pin is None else r.random(nv) < pin
    same_csr(f, nv, engine)
    same_smooth(v, f, factors, engine, pinned)
    seeds = r.integers(0, nv, int(r.integers(0, 4)))
    max_ring = int(r.integers(0, 6))
    got, info = ccta.vertex_rings_info(f, seeds, max_ring, nv, engine=engine)
    want, winfo = SMO.rings(f, nv, seeds, max_ring)
    assert np.array_equal(got, want) and info == winfo


# ---- errors ---------------------------------------------------------------------------------------------------------------

def test_errors(engine):
    N = mm._native
    L = N.lib()
    v, f = octahedron()
    f = np.ascontiguousarray(f, dtype=np.int64)
    with pytest.raises(ValueError, match="out of range"):
        mm.smooth_mesh((v, [[0, 1, 6]]), engine=engine)
    with pytest.raises(ValueError, match="out of range"):
        mm.vertex_rings(f, [6], 1, 6, engine=engine)
    with pytest.raises(ValueError, match="negative"):
        mm.smooth_mesh((v, f), iterations=-1, engine=engine)
    with pytest.raises(ValueError, match="negative"):
        mm.vertex_rings(f, [0], -1, 6, engine=engine)
    out, rep, fac = np.full((6, 3), 7.0), N.MMSmoothReport(), np.array([0.5])
    bad = f.copy()
    bad[3, 1] = 6
    call = lambda faces, n_steps, report: L.mm_mesh_smooth(engine.handle, N._ptr(v), 6, N._ptr(faces), 8, N._ptr(fac),   # noqa: E731
                                                           n_steps, None, N._ptr(out), report)
    assert call(bad, 1, C.byref(rep)) == -2 and call(f, -1, C.byref(rep)) == -2 and call(f, 1, None) == -2
    assert (out == 7.0).all()
    assert call(f, 1, C.byref(rep)) == 0 and rep.n_edges == 12
    off, nb, info = np.full(7, 7, dtype=np.int64), np.full(23, 7, dtype=np.int64), np.zeros(4, dtype=np.int64)
    rc = L.mm_mesh_adjacency_csr(engine.handle, N._ptr(f), 8, 6, 23, N._ptr(off), N._ptr(nb), N._ptr(info))
    assert rc == -3 and info.tolist() == [24, 4, 0, 7] and (off == 7).all() and (nb == 7).all()
    nb = np.zeros(24, dtype=np.int64)
    rc = L.mm_mesh_adjacency_csr(engine.handle, N._ptr(f), 8, 6, 24, N._ptr(off), N._ptr(nb), N._ptr(info))
    assert rc == 0 and off.tolist() == [0, 4, 8, 12, 16, 20, 24]
    ring, rinfo, seeds = np.zeros(6, dtype=np.int32), np.zeros(3, dtype=np.int64), np.array([6], dtype=np.int64)
    assert L.mm_mesh_vertex_rings(engine.handle, N._ptr(f), 8, 6, N._ptr(seeds), 1, 1, N._ptr(ring), N._ptr(rinfo)) == -2
    seeds[0] = 0
    assert L.mm_mesh_vertex_rings(engine.handle, N._ptr(f), 8, 6, N._ptr(seeds), 1, -1, N._ptr(ring), N._ptr(rinfo)) == -2
    assert L.mm_mesh_vertex_rings(engine.handle, N._ptr(f), 8, 6, N._ptr(seeds), 1, 5, N._ptr(ring), N._ptr(rinfo)) == 0
    assert ring.tolist() == [0, 2, 1, 1, 1, 1] and rinfo.tolist() == [6, 3, 7 + 1 + 3]


# ---- the line label -> remove -> stitch -----------------------------------------------------------------------------------

def test_stitch_with_and_without_smoothing(engine):
    res, geom, frames = takeoff_case(engine)
    plain = mm.stitch(dict(res), geom, region_remove="section_points", engine=engine, fill_holes=True)
    again = mm.stitch(dict(res), geom, region_remove="section_points", engine=engine, fill_holes=True, smooth=False)
    assert "smooth_report" not in plain and sorted(plain) == sorted(again)
    assert same_bits(plain["mesh"][0], again["mesh"][0]) and np.array_equal(plain["mesh"][1], again["mesh"][1])
    wv, wf, _ = CM.fill_holes(*mm.stitch(dict(res), geom, region_remove="section_points", engine=engine)["mesh"])
    assert same_bits(plain["mesh"][0], wv) and np.array_equal(plain["mesh"][1], wf)      # the parent's answer

    smooth = mm.stitch(dict(res), geom, region_remove="section_points", engine=engine, fill_holes=True, smooth=True)
    want, wrep = mm.smooth_mesh(plain["mesh"], engine=engine)
    assert same_bits(smooth["mesh"][0], want[0]) and np.array_equal(smooth["mesh"][1], plain["mesh"][1])
    assert smooth["smooth_report"] == wrep and wrep["steps_run"] == 10
    check, crep = SMO.smooth(*plain["mesh"], TAUBIN10)
    assert same_bits(want[0], check) and bits_equal(wrep["volume_after"], crep["volume_after"])
    assert wrep["volume_ratio"] == wrep["volume_after"] / wrep["volume_before"]
    _, n_open, n_nonmanifold = SM.face_adjacency(smooth["mesh"][1])
    assert n_open == 0 and n_nonmanifold == 0 and smooth["fill_report"] == plain["fill_report"]
    synced = ccta.sync_results_to_mesh(plain, plain["mesh"], want)
    moved = 0
    for key in ccta.SYNC_KEYS:
        if key in plain and len(plain[key]):
            assert same_bits(smooth[key], synced[key]) and len(smooth[key]) > 0
            assert (ccta._match(smooth["mesh"][0], smooth[key]) >= 0).all()             # they sit on the new mesh
            moved += not same_bits(smooth[key], plain[key])
    assert moved > 0

    # a dict of keywords: only a band of 2 edges around the proximal rim moves
    seeds = plain["prox_boundary_points"]
    banded = mm.stitch(dict(res), geom, region_remove="section_points", engine=engine, fill_holes=True,
                       smooth={"band": (seeds, 2), "iterations": 4})
    bwant, brep = mm.smooth_mesh(plain["mesh"], band=(seeds, 2), iterations=4, engine=engine)
    assert same_bits(banded["mesh"][0], bwant[0]) and banded["smooth_report"] == brep and brep["steps_run"] == 4
    still = (banded["mesh"][0] == plain["mesh"][0]).all(axis=1)
    assert 0 < brep["n_pinned"] == int(still.sum()) < len(still)

    cond = mm.stitch_conditioned(dict(res), geom, region_remove="section_points", engine=engine, fill_holes=True)
    cond_s = mm.stitch_conditioned(dict(res), geom, region_remove="section_points", engine=engine, fill_holes=True,
                                   smooth=True)
    cwant, crep2 = mm.smooth_mesh(cond["mesh"], engine=engine)
    assert same_bits(cond_s["mesh"][0], cwant[0]) and cond_s["smooth_report"] == crep2 and "smooth_report" not in cond
