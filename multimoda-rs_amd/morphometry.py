"""Lumen morphometry: the reference's per-contour measures (src/types/native/contour.rs:227-361: area, farthest
points, closest opposite points in 2-D and 3-D, elliptic ratio) and the summaries built on them
(src/types/binding/py_geometry.rs:190-260 ``PyGeometry.get_summary``, py_geometry_pair.rs:70-200
``PyGeometryPair.get_summary`` with its deformation table).

Every call measures all its contours in ONE device launch (``mm_contour_measures``, csrc/mm_shape_kernels.hip, exact
f64 with the reference's tie and NaN rules); the summary rule is host C (``mm_summary_from_measures``), so a C host
gets the same numbers.  Where the reference panics (the farthest points of an empty contour, a closest opposite or an
elliptic ratio below 3 points, a pair whose second geometry has fewer frames) these functions raise RuntimeError.

``tree_summary`` (``DiscretizedVesselTree.get_summary``) has no reference counterpart: it applies the reference's
geometry-summary rule and measures to the slices of a discretised CCTA vessel tree.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _native as N

MEASURE_CLOSEST_2D = 1          # MM_MEASURE_CLOSEST_2D (include/mm_build.h)
TABLE_HEADERS = ("id", "area_dia", "ellip_dia", "area_sys", "ellip_sys", "z")
TREE_TABLE_HEADERS = ("id", "area", "elliptic_ratio", "major", "minor_3d", "z")

GeomSummary = Tuple[float, float, float]


@dataclass
class ContourMeasures:
    """Per-contour measures of a batch, in input order.  Pairs are contour-local point indices in the reference's
    orientation; where the reference panics a value is NaN and its pair (-1, -1), and a skipped 2-D pass likewise."""
    n_points: np.ndarray         # (n,) int64
    area: np.ndarray             # (n,) Contour::area
    major: np.ndarray            # (n,) find_farthest_points distance
    major_pair: np.ndarray       # (n, 2) int64
    minor_3d: np.ndarray         # (n,) find_closest_opposite_3d distance
    minor_3d_pair: np.ndarray
    minor_2d: np.ndarray         # (n,) find_closest_opposite distance (NaN unless closest_2d)
    minor_2d_pair: np.ndarray
    elliptic_ratio: np.ndarray   # (n,)

    def __len__(self) -> int:
        return int(self.n_points.shape[0])


def _engine(engine: Optional[N.Engine]) -> N.Engine:
    if engine is not None:
        return engine
    from .api import default_engine
    return default_engine()


def _p3(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, 3))


def measure_csr(off: np.ndarray, xyz: np.ndarray, has_centroid: Optional[np.ndarray] = None,
                centroids: Optional[np.ndarray] = None, closest_2d: bool = False,
                engine: Optional[N.Engine] = None) -> ContourMeasures:
    """``mm_contour_measures`` on CSR contours: contour c = xyz[off[c]:off[c+1]].  The 2-D pass centres contour c on
    centroids[c] where has_centroid[c] is set, else on the mean of its points."""
    off = np.ascontiguousarray(off, dtype=np.int64)
    xyz = _p3(xyz)
    n = off.shape[0] - 1
    if n < 0 or int(off[-1]) != xyz.shape[0]:
        raise ValueError("measure_csr: the offsets do not match the points")
    hc = cen = None
    if has_centroid is not None:
        hc = np.ascontiguousarray(has_centroid, dtype=np.uint8).reshape(n)
        cen = np.ascontiguousarray(centroids, dtype=np.float64).reshape(n, 3)
    val = np.zeros((n, 5))
    idx = np.zeros((n, 6), dtype=np.int64)
    N.check(N.lib().mm_contour_measures(_engine(engine).handle, n, N._ptr(off), N._ptr(xyz), N._ptr(hc), N._ptr(cen),
                                        MEASURE_CLOSEST_2D if closest_2d else 0, N._ptr(val), N._ptr(idx)),
            "contour_measures")
    return ContourMeasures(np.diff(off), val[:, 0].copy(), val[:, 1].copy(), idx[:, 0:2].copy(), val[:, 2].copy(),
                           idx[:, 2:4].copy(), val[:, 3].copy(), idx[:, 4:6].copy(), val[:, 4].copy())


def _csr(contours):
    """frames.Contour objects or (n, 3) arrays -> (off, xyz, has_centroid, centroids)"""
    pts, hc, cen = [], [], []
    for c in contours:
        p = getattr(c, "points", c)
        pts.append(_p3(p))
        cc = getattr(c, "centroid", None)
        hc.append(cc is not None)
        cen.append(cc if cc is not None else (0.0, 0.0, 0.0))
    off = np.zeros(len(pts) + 1, dtype=np.int64)
    off[1:] = np.cumsum([p.shape[0] for p in pts])
    xyz = np.ascontiguousarray(np.concatenate(pts)) if pts else np.zeros((0, 3))
    return off, xyz, np.array(hc, dtype=np.uint8), np.array(cen, dtype=np.float64).reshape(-1, 3)


def contour_measures(contours: Sequence, closest_2d: bool = True, engine: Optional[N.Engine] = None) -> ContourMeasures:
    """Area, major axis (farthest points), 3-D and 2-D minor axes (closest opposite points) and elliptic ratio of every
    contour (``frames.Contour`` objects or (n, 3) point arrays), in one device launch.  The 2-D pass
    (``find_closest_opposite``) centres a contour on its stored centroid, or on the mean of its points where it has
    none (arrays have none); ``closest_2d=False`` skips it."""
    off, xyz, hc, cen = _csr(contours)
    return measure_csr(off, xyz, hc, cen, closest_2d, engine)


def summary_from_measures(area, ratio, n_points, centroids) -> GeomSummary:
    """PyGeometry::get_summary's rule (py_geometry.rs:190-260) on per-frame lumen areas, elliptic ratios, point counts
    and frame centroids: ``(mla, max_stenosis, stenosis_length_mm)``, host C (``mm_summary_from_measures``)."""
    area = np.ascontiguousarray(area, dtype=np.float64).reshape(-1)
    F = area.shape[0]
    ratio = np.ascontiguousarray(ratio, dtype=np.float64).reshape(F)
    n_points = np.ascontiguousarray(n_points, dtype=np.int64).reshape(F)
    centroids = np.ascontiguousarray(centroids, dtype=np.float64).reshape(F, 3)
    out = np.zeros(3)
    N.check(N.lib().mm_summary_from_measures(F, N._ptr(area), N._ptr(ratio), N._ptr(n_points), N._ptr(centroids),
                                             N._ptr(out)), "get_summary")
    return float(out[0]), float(out[1]), float(out[2])


def _lumen_z(g) -> np.ndarray:
    """The lumen contour centroid's z per frame (PyContour.centroid, None -> 0.0: py_contour.rs:427)."""
    z = np.zeros(g.n_frames)
    if g.lumen_centroids is not None:
        has = np.ones(g.n_frames, dtype=bool) if g.has_lumen_centroid is None else g.has_lumen_centroid.astype(bool)
        z[has] = g.lumen_centroids[has, 2]
    return z


def geometry_summary(g, engine: Optional[N.Engine] = None) -> GeomSummary:
    """``FlatGeometry.get_summary`` (py_geometry.rs:190-260): lumen areas and elliptic ratios in one launch, then the
    summary rule with the frame centroids."""
    if g.n_frames == 0:
        return 0.0, 0.0, 0.0
    m = measure_csr(g.lumen_off, g.lumen, engine=engine)
    return summary_from_measures(m.area, m.elliptic_ratio, m.n_points, g.centroids)


def _need_ratio(m: ContourMeasures, what: str) -> None:
    bad = np.nonzero(m.n_points < 3)[0]
    if bad.size:
        k = int(bad[0])
        why = "is empty" if m.n_points[k] == 0 else "has fewer than 3 points"
        raise RuntimeError(f"{what}: lumen contour {k} {why}: its elliptic ratio is undefined")


def _fmt2(v: float) -> str:
    """Rust's format!("{:.2}", v): correctly rounded like Python's, but NaN prints as NaN."""
    return "NaN" if v != v else "%.2f" % v


def format_table(ids, columns, headers=TABLE_HEADERS) -> str:
    """The bordered table create_deformation_table prints (py_geometry_pair.rs:127-196): centred header, left-aligned
    cells, ``{:.2}`` floats and the id as an integer."""
    rows = [[str(int(i))] + [_fmt2(float(c[k])) for c in columns] for k, i in enumerate(ids)]
    widths = [len(h) for h in headers]
    for r in rows:
        widths = [max(w, len(c)) for w, c in zip(widths, r)]
    border = "+" + "".join("-" * (w + 2) + "+" for w in widths)
    head = "|"
    for h, w in zip(headers, widths):
        left = (w - len(h)) // 2
        head += " " + " " * left + h + " " * (w - len(h) - left) + " |"
    lines = [border, head, border]
    for r in rows:
        lines.append("|" + "".join(" " + c + " " * (w - len(c)) + " |" for c, w in zip(r, widths)))
    lines.append(border)
    return "\n".join(lines) + "\n"


def pair_summary(pair, print_table: bool = True, engine: Optional[N.Engine] = None):
    """``GeometryPair.get_summary`` (py_geometry_pair.rs:70-200): ``((summary_a, summary_b), table)`` with one row
    ``[lumen id, area_a, ellip_a, area_b, ellip_b, z]`` per frame of geom_a (z: the lumen contour centroid's z, 0.0
    where it has none).  Both geometries in one launch.  geom_b with fewer frames than geom_a is an error (a panic in
    the reference); its extra frames are ignored.  The table is printed as the reference prints it unless
    ``print_table`` is False."""
    a, b = pair.geom_a, pair.geom_b
    off = np.concatenate([a.lumen_off, b.lumen_off[1:] + a.lumen_off[-1]]).astype(np.int64)
    m = measure_csr(off, np.concatenate([a.lumen, b.lumen]), engine=engine)
    Fa, Fb = a.n_frames, b.n_frames
    sa = summary_from_measures(m.area[:Fa], m.elliptic_ratio[:Fa], m.n_points[:Fa], a.centroids)
    sb = summary_from_measures(m.area[Fa:], m.elliptic_ratio[Fa:], m.n_points[Fa:], b.centroids)
    _need_ratio(m, "GeometryPair.get_summary")
    if Fb < Fa:
        raise RuntimeError(f"GeometryPair.get_summary: geom_b has {Fb} frames, fewer than geom_a's {Fa}")
    ids = a.lumen_ids.astype(np.float64)
    table = np.stack([ids, m.area[:Fa], m.elliptic_ratio[:Fa], m.area[Fa:2 * Fa], m.elliptic_ratio[Fa:2 * Fa],
                      _lumen_z(a)], axis=1).reshape(Fa, 6)
    if print_table:
        print(format_table(a.lumen_ids, [table[:, k] for k in range(1, 6)]), end="")
    return (sa, sb), table


def _vessel(m: ContourMeasures, s: slice, contours) -> tuple:
    if not contours:
        return (0.0, 0.0, 0.0), np.zeros((0, 6))
    cen = np.array([c.centroid if c.centroid is not None else tuple(np.mean(c.points, axis=0)) for c in contours],
                   dtype=np.float64).reshape(-1, 3)
    summary = summary_from_measures(m.area[s], m.elliptic_ratio[s], m.n_points[s], cen)
    ids = np.array([c.id for c in contours], dtype=np.float64)
    table = np.stack([ids, m.area[s], m.elliptic_ratio[s], m.major[s], m.minor_3d[s], cen[:, 2]], axis=1)
    return summary, table


def tree_summary(tree, engine: Optional[N.Engine] = None) -> dict:
    """``DiscretizedVesselTree.get_summary``: the geometry-summary rule and a per-slice table ``[id, area,
    elliptic_ratio, major, minor_3d, z]`` for the aorta, both main vessels and every side branch, each slice's
    centroid (its anchor) standing in for the frame centroid.  Every slice of the tree goes through one launch.  Not a
    reference function: it composes the reference's measures (contour.rs) and summary rule (py_geometry.rs:190-260).
    Returns ``{"aorta": (summary, table), "rca_main": ..., "lca_main": ..., "rca_branches": [...],
    "lca_branches": [...]}``."""
    vessels = [tree.discretized_aorta, tree.discretized_rca_main, tree.discretized_lca_main,
               *tree.rca_branches, *tree.lca_branches]
    m = contour_measures([c for v in vessels for c in v], closest_2d=False, engine=engine)
    _need_ratio(m, "DiscretizedVesselTree.get_summary")
    out, k = [], 0
    for v in vessels:
        out.append(_vessel(m, slice(k, k + len(v)), v))
        k += len(v)
    nr = len(tree.rca_branches)
    return {"aorta": out[0], "rca_main": out[1], "lca_main": out[2], "rca_branches": out[3:3 + nr],
            "lca_branches": out[3 + nr:]}


# ---- one contour (frames.Contour methods) ---------------------------------------------------------------------------
def _one(contour, closest_2d: bool, engine) -> ContourMeasures:
    return contour_measures([contour], closest_2d=closest_2d, engine=engine)


def _pt(p, k: int) -> Tuple[float, float, float]:
    return float(p[k, 0]), float(p[k, 1]), float(p[k, 2])


def get_area(contour, engine: Optional[N.Engine] = None) -> float:
    """Contour::area (contour.rs:345-361); 0.0 below 3 points."""
    if len(contour.points) < 3:
        return 0.0
    return float(_one(contour, False, engine).area[0])


def find_farthest_points(contour, engine: Optional[N.Engine] = None):
    """Contour::find_farthest_points (contour.rs:227-242): ``((p1, p2), distance)``, points as (x, y, z)."""
    if len(contour.points) == 0:
        raise RuntimeError("find_farthest_points: the contour has no points")
    m = _one(contour, False, engine)
    i, j = (int(v) for v in m.major_pair[0])
    return (_pt(contour.points, i), _pt(contour.points, j)), float(m.major[0])


def find_closest_opposite(contour, engine: Optional[N.Engine] = None):
    """Contour::find_closest_opposite (contour.rs:247-310), centred on the stored centroid or else on the mean of
    the points: ``((p1, p2), distance)``."""
    if len(contour.points) < 3:
        raise RuntimeError("find_closest_opposite: need at least 3 points")
    m = _one(contour, True, engine)
    i, j = (int(v) for v in m.minor_2d_pair[0])
    return (_pt(contour.points, i), _pt(contour.points, j)), float(m.minor_2d[0])


def get_elliptic_ratio(contour, engine: Optional[N.Engine] = None) -> float:
    """Contour::elliptic_ratio (contour.rs:335-343): farthest distance against the 3-D closest opposite distance."""
    n = len(contour.points)
    if n < 3:
        raise RuntimeError("get_elliptic_ratio: " + ("the contour has no points" if n == 0 else
                                                     "need at least 3 points"))
    return float(_one(contour, False, engine).elliptic_ratio[0])
