"""Sliver faces on the device (csrc/mm_tri_device.h through csrc/mm_tri_kernels.hip and csrc/mm_relax_kernels.hip): the
cases of tests/tri_sliver_cases.py against the checker, bit for bit -- every per-face family as one small mesh, faces
either side of the thin rule's threshold among them, so the staging's kind and the checker's face_kind must agree; the
strip, whose pass B must skip items; the squeezed tube; the strip with its faces shuffled -- then a property that does not
lean on the checker (a mesh is at distance 0 from itself, up to the thin rule's allowance), and the relaxation's seeds and
projections on the same meshes.  The bounds are those of tests/test_surface_sliver_host.py."""
import numpy as np
import pytest

from mm_checkers import relax_mesh as RX
from test_refine_host import same_bits, wound_tube
from test_surface_host import must_skip
from test_surface_sliver_host import R_TOL, scale_of, sliver_meshes, thin_altitude
from test_gpu_surface import same_as_checker
from test_gpu_relax import bits, same_relax
import tri_sliver_cases as C

import multimoda_rs_amd as mm
from multimoda_rs_amd import surface

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def meshes():
    return sliver_meshes()


@pytest.mark.parametrize("name", ["cap_axis", "cap_random", "collinear", "needle_axis", "needle_random"])
def test_families_against_the_checker(engine, name):
    v, f, q = C.families()[name]
    got = same_as_checker(q.reshape(-1, 3), v, f, engine)                 # every query against every face of the family
    assert np.isfinite(got.sq_distance).all() and np.isfinite(got.closest).all()
    assert set(got.region.tolist()) <= {0, 1, 2, 3, 4, 5, 6}


def test_strip_skips_what_it_must_and_equals_the_unpruned_scan(engine, meshes):
    v, f, q = meshes["strip"]
    n = must_skip(surface.tri_plan(q, (v, f)), q, v, f)
    got = same_as_checker(q, v, f, engine)
    print(f"strip: pass B {got.report['items_pass_b']} items, skipped {got.report['items_skipped']}, must_skip {n}")
    assert got.report["items_skipped"] >= n > 0 and got.report["n_launches"] == 5


def test_squeezed_tube_against_the_checker(engine, meshes):
    v, f, q = meshes["tube"]
    got = same_as_checker(q, v, f, engine)
    assert got.report["items_pass_a"] >= 3 and got.report["items_pass_b"] == 3 * got.report["items_pass_a"]


def test_strip_with_shuffled_faces(engine, meshes):
    v, f, q = meshes["strip"]
    perm = np.random.default_rng(13).permutation(len(f))
    base = mm.point_mesh_distance(q, (v, f), engine=engine)
    other = same_as_checker(q, v, f[perm], engine)
    assert same_bits(base.sq_distance, other.sq_distance)


@pytest.mark.parametrize("name", ["strip", "tube"])
def test_a_mesh_is_on_itself(engine, meshes, name):
    v, f, _ = meshes[name]
    rep = mm.surface_distance((v, f), (v, f), samples=2, engine=engine)
    allow = thin_altitude(v, f)[1] + R_TOL * scale_of(v)
    print(f"{name}: Hausdorff distance to itself {rep.hausdorff:.3e}, allowance {allow:.3e}")
    assert 0.0 <= rep.hausdorff <= allow and rep.a_to_b.n == 6 * len(f)


def test_projection_of_the_strips_queries(engine, meshes):
    """project_to_mesh needs free vertices: the queries take the places of the vertices of a closed tube."""
    v, f, q = meshes["strip"]
    _, tf = wound_tube(12, 85)
    tv = q[:tf.max() + 1]
    assert len(tv) == 12 * 85 + 2 > 1000
    (pv, _), face, rep = mm.project_to_mesh((tv, tf), (v, f), engine=engine)
    wv, wface, wrep = RX.relax(tv, tf, v, f, iterations=0)[:3]
    assert same_bits(pv, wv) and np.array_equal(face, wface) and (face >= 0).all()
    assert bits(rep["initial_distance_sq"]) == bits(wrep["initial_distance_sq"]) and rep["n_free"] == len(tv)


def test_one_relaxation_step_on_the_squeezed_tube(engine):
    v, f = C.squeezed_tube()
    _, face, rep = same_relax((v, f), None, engine, iterations=1)
    assert rep["n_free"] == len(v) and (face >= 0).all()
