"""multimoda-rs_amd -- MI355X-native Hausdorff pose-search engine.

One hot path of yungselm/multimoda-rs (the brute-force / coarse-to-fine Hausdorff rotation
search of ``src/intravascular``) rebuilt for gfx950: hand-written HIP kernels behind a
C ABI (``include/mm_hausdorff.h``), host orchestration in C++, and this thin Python layer
that mirrors the reference's ``mm.from_array_*`` / ``mm.from_file_*`` entry points for
that path.  Import as ``import multimoda_rs_amd as mm`` (root-level shim), since the
package directory name contains a hyphen.
"""
from __future__ import annotations

from . import _native
from ._native import (MM_PRECISION_F32, MM_PRECISION_F32_BOUNDED, MM_PRECISION_F32_FAST, MM_PRECISION_F32_MATRIX, MM_PRECISION_F64, MM_SEARCH_SKIP_ZERO, Batch, Comm, Engine,
                      IndexedBatch, Plan,
                      device_count, filter_points_in_region, refine_angles, refine_downsample_count, search_angles)
from .geometry import (FlatGeometry, WithinPlan, align_between, align_within, between_points, catheter_points,
                       contour_centroid, search_set)
from .io import InputData, Record, build_geometry_from_inputdata, numpy_to_inputdata, process_directory
from .api import (GeometryPair, align_frames_in_geometries, from_array_doublepair, from_array_full,
                  from_array_single, from_array_singlepair, from_file_doublepair, from_file_full,
                  from_file_single, from_file_singlepair)
from .centerline import (Centerline, align_combined, align_manual, align_three_point, numpy_to_centerline, read_centerline_vtp,
                         preprocess_centerline, load_centerline, prepare_centerline)
from . import centerline
from . import ccta
from .ccta import (DiscretizedVesselTree, adjust_diameter_centerline_morphing_simple, clean_outlier_points,
                   discretize_vessel, discretize_vessel_tree, final_reclassification,
                   BSplineReport, discretize_vessel_tree_bspline, fit_bspline_contour, fit_bspline_contours,
                   replace_contours_with_bsplines,
                   find_aorta_scaling, find_aortic_points, find_aortic_scaling, find_aortic_wall_scaling,
                   find_centerline_bounded_points_simple, find_distal_and_proximal_scaling, find_faces_near_points,
                   find_points_by_cl_region, find_proximal_distal_scaling, keep_largest_connected_component,
                   label_anomalous_region, label_geometry, remove_occluded_points_ray_triangle, scale,
                   scale_region_centerline_morphing, sync_results_to_mesh, open_boundary_edges, order_boundary_rings,
                   clean_open_boundary, remove_labeled_points_from_mesh, keep_labeled_points_from_mesh,
                   extract_region_with_border_faces, export_section_stl, build_adjacency_map,
                   fix_mesh_winding, assemble_mesh, stitch_rings, stitch_ccta_to_intravascular, stitch, branch_masks,
                   label_branches, label_branches_pair, find_sharp_angles, label, manual_hole_fill, fill_holes,
                   smooth_mesh_labels, create_wall_mesh, condition_boundary_rings, stitch_conditioned, smooth_mesh,
                   filter_taubin, filter_laplacian, mesh_adjacency_csr, vertex_rings, postprocess_stitched_mesh,
                   mesh_edge_lengths, edge_length_target, refine_mesh, relax_mesh, project_to_mesh,
                   mesh_valence, flip_edges, collapse_edges, isotropic_remesh, repair_mesh,
                   mesh_manifold_report, fix_and_remesh_stitched_mesh)
from . import surface
from .surface import (DirectedDistance, PointMeshDistance, SurfaceDistanceReport, point_mesh_distance,
                      sample_mesh_surface, surface_distance)
from . import intersect
from .intersect import MeshIntersections, mesh_intersections, mesh_self_intersections
from . import section
from .section import MeshCrossSections, VesselProfile, centerline_cross_sections, mesh_cross_sections, vessel_profile
from . import clip
from .clip import ClipError, ClippedMesh, clip_mesh, open_vessel_ends, vessel_end_stations
from . import winding
from .winding import (ContainmentReport, IntramuralCourse, IntramuralPoints, SignedPointMeshDistance, WindingNumber,
                      intramural_course, intramural_points, mesh_containment, mesh_winding_number, points_in_mesh,
                      signed_point_mesh_distance)
from . import skeleton
from .skeleton import SkeletonGraph, centerline_from_mesh, mesh_geodesic_distance, mesh_skeleton, skeleton_centerline
from .convert import numpy_to_geometry, to_array
from . import morphometry
from .morphometry import ContourMeasures, contour_measures
from .export import to_obj
from . import export
from .extension import ShiftRotationSearch
from .synth import synthetic_case, synthetic_pullback

__version__ = "0.1.0"

__all__ = [
    "Engine", "Comm", "Batch", "Plan", "FlatGeometry", "device_count", "search_angles", "refine_angles",
    "filter_points_in_region", "refine_downsample_count",
    "align_within", "align_between", "WithinPlan", "search_set", "between_points",
    "from_file_full", "from_file_doublepair", "from_file_singlepair", "from_file_single",
    "from_array_full", "from_array_doublepair", "from_array_singlepair", "from_array_single",
    "InputData", "Record", "numpy_to_inputdata", "build_geometry_from_inputdata", "process_directory",
    "GeometryPair", "align_frames_in_geometries",
    "ShiftRotationSearch", "to_array", "numpy_to_geometry", "to_obj", "export",
    "Centerline", "numpy_to_centerline", "read_centerline_vtp", "preprocess_centerline", "align_three_point", "align_manual",
    "align_combined", "centerline",
    "ccta", "adjust_diameter_centerline_morphing_simple", "find_proximal_distal_scaling", "find_aortic_scaling",
    "find_aortic_wall_scaling", "find_distal_and_proximal_scaling", "find_aorta_scaling",
    "find_points_by_cl_region", "clean_outlier_points",
    "find_centerline_bounded_points_simple", "find_faces_near_points", "remove_occluded_points_ray_triangle",
    "find_aortic_points", "final_reclassification", "label_geometry",
    "discretize_vessel", "discretize_vessel_tree", "DiscretizedVesselTree",
    "BSplineReport", "discretize_vessel_tree_bspline", "fit_bspline_contour", "fit_bspline_contours",
    "replace_contours_with_bsplines",
    "keep_largest_connected_component", "label_anomalous_region", "scale_region_centerline_morphing",
    "sync_results_to_mesh", "scale", "open_boundary_edges", "order_boundary_rings", "clean_open_boundary",
    "remove_labeled_points_from_mesh", "keep_labeled_points_from_mesh", "extract_region_with_border_faces",
    "export_section_stl", "build_adjacency_map",
    "fix_mesh_winding", "assemble_mesh", "stitch_rings", "stitch_ccta_to_intravascular", "stitch",
    "load_centerline", "prepare_centerline", "branch_masks", "label_branches", "label_branches_pair", "find_sharp_angles",
    "label", "manual_hole_fill", "fill_holes", "smooth_mesh_labels", "create_wall_mesh",
    "condition_boundary_rings", "stitch_conditioned",
    "smooth_mesh", "filter_taubin", "filter_laplacian", "mesh_adjacency_csr", "vertex_rings", "postprocess_stitched_mesh",
    "mesh_edge_lengths", "edge_length_target", "refine_mesh", "relax_mesh", "project_to_mesh",
    "mesh_valence", "flip_edges", "collapse_edges", "isotropic_remesh",
    "repair_mesh", "mesh_manifold_report", "fix_and_remesh_stitched_mesh",
    "surface", "point_mesh_distance", "sample_mesh_surface", "surface_distance", "PointMeshDistance",
    "DirectedDistance", "SurfaceDistanceReport",
    "intersect", "mesh_self_intersections", "mesh_intersections", "MeshIntersections",
    "section", "mesh_cross_sections", "centerline_cross_sections", "vessel_profile", "MeshCrossSections", "VesselProfile",
    "clip", "clip_mesh", "open_vessel_ends", "vessel_end_stations", "ClippedMesh", "ClipError",
    "winding", "mesh_winding_number", "points_in_mesh", "signed_point_mesh_distance", "mesh_containment",
    "intramural_points", "intramural_course", "WindingNumber", "SignedPointMeshDistance", "ContainmentReport",
    "IntramuralPoints", "IntramuralCourse",
    "skeleton", "mesh_geodesic_distance", "mesh_skeleton", "centerline_from_mesh", "skeleton_centerline", "SkeletonGraph",
    "morphometry", "ContourMeasures", "contour_measures",
    "synthetic_case", "synthetic_pullback", "catheter_points", "contour_centroid",
    "MM_PRECISION_F32", "MM_PRECISION_F32_BOUNDED", "MM_PRECISION_F32_FAST", "MM_PRECISION_F32_MATRIX", "MM_PRECISION_F64", "MM_SEARCH_SKIP_ZERO",
]
