"""Lumen morphometry without a GPU: the checker (tests/mm_checkers/morphometry.py) against the reference's own known
answers (src/types/native/contour.rs tests, build.rs test_rest_directory_area_elliptic), the host summary rule
(mm_summary_from_measures) against the checker bit for bit, and GeometryPair.get_summary's errors and printed table
(the measures are stubbed here; the GPU suite measures for real)."""
import math
import os

import numpy as np
import pytest

from mm_checkers import morphometry as MC

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SQUARE = [(0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (2.0, 2.0, 0.0), (0.0, 2.0, 0.0)]
OPPOSITE = [(0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (0.0, -0.5, 0.0), (-1.0, 0.0, 0.0)]
RHOMBUS = [(1.0, 0.0, 0.0), (0.0, 2.0, 0.0), (1.0, 4.0, 0.0), (2.0, 2.0, 0.0)]


@pytest.fixture(scope="module")
def built(mm):
    import __graft_entry__ as ge
    ge.build()
    return mm


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


# ---- the reference's known answers ------------------------------------------------------------------------------
def test_square_farthest_points_is_sqrt8():
    (i, j), d = MC.farthest_points(SQUARE)
    assert d == math.sqrt(8.0) and (i, j) == (0, 2)
    assert MC.farthest_points_np(SQUARE) == ((0, 2), d)


def test_closest_opposite_with_stored_centroid():
    (i, j), d = MC.closest_opposite(OPPOSITE, (0.0, 0.125, 0.0))
    assert abs(d - 1.5) < 1e-6 and {i, j} == {0, 2}


def test_rhombus_ratio_and_area_and_short_contours():
    assert abs(MC.elliptic_ratio(RHOMBUS) - 2.0) < 1e-6
    assert abs(MC.area(RHOMBUS) - 4.0) < 1e-6
    assert MC.area([(0.0, 0.0, 0.0), (3.0, 0.0, 0.0), (0.0, 4.0, 0.0)]) == 6.0
    assert MC.area([]) == 0.0 and MC.area(SQUARE[:2]) == 0.0
    with pytest.raises(MC.Panic):
        MC.farthest_points([])
    with pytest.raises(MC.Panic):
        MC.closest_opposite_3d(SQUARE[:2])
    with pytest.raises(MC.Panic):
        MC.closest_opposite(SQUARE[:2])


def test_rest_directory_frame0_known_answers(built):
    from multimoda_rs_amd import frames
    g = built.build_geometry_from_inputdata(None, os.path.join(GOLD, "ivus_rest"), "full", True)
    lum = frames.to_frames(g)[0].lumen
    assert int(g.orig_frames[0]) == 385
    assert MC.area(lum.points) == pytest.approx(5.42, abs=0.1)
    assert MC.farthest_points(lum.points)[1] == pytest.approx(5.2, abs=0.1)
    assert MC.closest_opposite(lum.points, lum.centroid)[1] == pytest.approx(1.15, abs=0.1)
    assert MC.elliptic_ratio(lum.points) == pytest.approx(4.52, abs=0.1)


@pytest.mark.parametrize("seed", range(6))
def test_vectorised_farthest_matches_the_scalar_fold(seed):
    r = np.random.default_rng(seed)
    n = int(r.integers(1, 40))
    p = r.normal(size=(n, 3))
    if seed % 2:
        p = np.round(p, 0)                                      # many equal distances
    if seed == 4:
        p[3] = np.nan
    if seed == 5:
        p[:] = 1.0                                              # all distances 0: pair (0, 0)
    assert MC.farthest_points_np(p) == MC.farthest_points(p)


@pytest.mark.parametrize("seed", range(6))
def test_vectorised_closest_opposite_matches_the_scalar_fold(seed):
    r = np.random.default_rng(seed)
    n = int(r.integers(3, 40))
    p = r.normal(size=(n, 3))
    if seed % 2:
        p = np.round(p, 0)                                      # duplicated points, equal angles
    if seed == 4:
        p[2] = np.nan
    cen = None if seed < 3 else tuple(r.normal(size=3))
    assert MC.closest_opposite_np(p, cen) == MC.closest_opposite(p, cen)


def test_near_tie_keeps_the_earlier_pair():
    """Two distinct squared distances with one sqrt: the reference keeps the earlier pair."""
    a = 1.0
    b = np.nextafter(1.0, 2.0)
    assert a != b and math.sqrt(a) == math.sqrt(b)
    p = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 0.0), (math.sqrt(b), 0.0, 0.0)]
    assert MC.farthest_points(p)[0] == MC.farthest_points_np(p)[0]


# ---- mm_summary_from_measures against the checker -----------------------------------------------------------------
def _summary_case(r, F, kind):
    area = r.uniform(0.5, 10.0, F)
    ratio = r.uniform(1.0, 1.6, F)
    if kind == "elliptic":
        ratio = r.uniform(1.0, 1.29, F)
    if kind == "nan":
        area[r.integers(0, F, max(F // 3, 1))] = np.nan
    if kind == "equal":
        area[:] = 3.25
    if kind == "allnan":
        area[:] = np.nan
    if kind == "zero":
        area[:] = 0.0
    cen = np.cumsum(r.uniform(0.1, 1.0, (F, 3)), axis=0)
    return area, ratio, np.full(F, 50, dtype=np.int64), cen


@pytest.mark.parametrize("kind", ["random", "elliptic", "nan", "equal", "allnan", "zero"])
@pytest.mark.parametrize("seed", range(4))
def test_summary_rule_bit_for_bit(built, kind, seed):
    from multimoda_rs_amd import morphometry
    r = np.random.default_rng(seed)
    F = int(r.integers(1, 60))
    area, ratio, npts, cen = _summary_case(r, F, kind)
    got = morphometry.summary_from_measures(area, ratio, npts, cen)
    want = MC.summary(area, lambda k: float(ratio[k]), cen)
    assert np.array_equal(bits(got), bits(want)) or (np.isnan(got).tolist() == np.isnan(want).tolist() and
                                                     np.array_equal(bits(np.nan_to_num(got)), bits(np.nan_to_num(want))))


def test_summary_zero_frames(built):
    from multimoda_rs_amd import morphometry
    assert morphometry.summary_from_measures([], [], [], np.zeros((0, 3))) == (0.0, 0.0, 0.0)
    assert MC.summary([], None, []) == (0.0, 0.0, 0.0)


def test_summary_short_contour_is_an_error_only_where_all_reaches_it(built):
    """Rust's all() stops at the first ratio >= 1.3: a frame of 2 points behind it is never measured; before it, it is
    the reference's panic."""
    from multimoda_rs_amd import morphometry
    area = np.array([4.0, 3.0, 0.0, 5.0])
    cen = np.arange(12, dtype=np.float64).reshape(4, 3)
    npts = np.array([50, 50, 2, 50])
    ratio = np.array([1.1, 1.5, np.nan, 1.1])                   # frame 1 stops the test: frame 2 is not reached
    got = morphometry.summary_from_measures(area, ratio, npts, cen)
    assert got == MC.summary(area, lambda k: float(ratio[k]), cen)
    ratio[1] = 1.2                                              # now frame 2 is reached
    with pytest.raises(RuntimeError, match="fewer than 3 points"):
        morphometry.summary_from_measures(area, ratio, npts, cen)
    npts[2] = 0
    with pytest.raises(RuntimeError, match="empty lumen contour"):
        morphometry.summary_from_measures(area, ratio, npts, cen)


def test_summary_null_arguments_are_invalid(built):
    L = built._native.lib()
    assert L.mm_summary_from_measures(0, None, None, None, None, None) == -2
    out = np.zeros(3)
    assert L.mm_summary_from_measures(2, None, None, None, None, built._native._ptr(out)) == -2
    assert L.mm_summary_from_measures(-1, None, None, None, None, built._native._ptr(out)) == -2
    assert L.mm_contour_measures(None, 1, None, None, None, None, 0, None, None) == -2


# ---- GeometryPair.get_summary: errors and the printed table (measures stubbed) -----------------------------------------
def _stub_measures(monkeypatch, morphometry):
    """The device pass replaced by the checker (the GPU suite compares the two)."""
    def measure_csr(off, xyz, has_centroid=None, centroids=None, closest_2d=False, engine=None):
        off = np.asarray(off, dtype=np.int64)
        rows = [MC.measures(xyz[off[c]:off[c + 1]], closest_2d=False) for c in range(off.shape[0] - 1)]
        col = lambda k: np.array([r[k] for r in rows], dtype=np.float64)
        pair = lambda k: np.array([r[k] for r in rows], dtype=np.int64).reshape(-1, 2)
        return morphometry.ContourMeasures(np.diff(off), col("area"), col("major"), pair("major_pair"),
                                           col("minor_3d"), pair("minor_3d_pair"), col("minor_2d"),
                                           pair("minor_2d_pair"), col("elliptic_ratio"))
    monkeypatch.setattr(morphometry, "measure_csr", measure_csr)


def _ring_geometry(mm, F, n=24, seed=0, ids=None):
    r = np.random.default_rng(seed)
    t = np.linspace(0, 2 * np.pi, n, endpoint=False)
    lum = []
    for k in range(F):
        a, b = r.uniform(0.8, 2.0), r.uniform(0.8, 2.0)
        lum.append(np.stack([a * np.cos(t), b * np.sin(t), np.full(n, 0.5 * k)], 1))
    g = mm.FlatGeometry.from_frames(lum, ids=ids)
    return g


def test_pair_summary_table_and_printout(built, monkeypatch, capsys):
    from multimoda_rs_amd import morphometry
    _stub_measures(monkeypatch, morphometry)
    a = _ring_geometry(built, 7, seed=1, ids=[3, 4, 5, 6, 7, 8, 1000])
    b = _ring_geometry(built, 9, seed=2)                        # extra frames of geom_b are ignored
    a.lumen_centroids = a.centroids.copy() + 0.25
    a.has_lumen_centroid = np.array([1, 1, 0, 1, 1, 1, 1], dtype=np.uint8)
    a.lumen[0, 0] = np.nan                                      # a NaN cell prints as NaN
    pair = built.GeometryPair(a, b)
    (sa, sb), table = pair.get_summary()
    text = capsys.readouterr().out
    lum = lambda g: [g.frame_lumen(i) for i in range(g.n_frames)]
    assert sa == MC.geometry_summary(lum(a), a.centroids) and sb == MC.geometry_summary(lum(b), b.centroids)
    ea = [MC.elliptic_ratio(p) for p in lum(a)]
    eb = [MC.elliptic_ratio(p) for p in lum(b)][:7]
    z = [a.lumen_centroids[i, 2] if a.has_lumen_centroid[i] else 0.0 for i in range(7)]
    want = np.array([[a.lumen_ids[i], MC.area(lum(a)[i]), ea[i], MC.area(lum(b)[i]), eb[i], z[i]] for i in range(7)])
    assert table.shape == (7, 6) and np.array_equal(np.isnan(table), np.isnan(want))
    assert np.array_equal(np.nan_to_num(table), np.nan_to_num(want))
    assert text == MC.deformation_table_text(a.lumen_ids, want[:, 1], want[:, 2], want[:, 3], want[:, 4], want[:, 5])
    assert "NaN" in text and "| 1000 |" in text
    pair.get_summary(print_table=False)
    assert capsys.readouterr().out == ""


def test_pair_summary_errors(built, monkeypatch):
    from multimoda_rs_amd import morphometry
    _stub_measures(monkeypatch, morphometry)
    a, b = _ring_geometry(built, 6, seed=3), _ring_geometry(built, 5, seed=4)
    with pytest.raises(RuntimeError, match="fewer than geom_a"):
        built.GeometryPair(a, b).get_summary(print_table=False)
    short = built.FlatGeometry.from_frames([a.frame_lumen(i) if i != 5 else a.frame_lumen(i)[:2] for i in range(6)])
    with pytest.raises(RuntimeError, match="fewer than 3 points"):
        built.GeometryPair(short, _ring_geometry(built, 6)).get_summary(print_table=False)


def test_table_header_is_centred():
    text = MC.deformation_table_text([12345678], [1.0], [1.0], [1.0], [1.0], [-0.001])
    lines = text.splitlines()
    assert lines[1].startswith("|    id    |") and "-0.00" in lines[3]
    from multimoda_rs_amd import morphometry
    assert morphometry.format_table([12345678], [[1.0], [1.0], [1.0], [1.0], [-0.001]]) == text
