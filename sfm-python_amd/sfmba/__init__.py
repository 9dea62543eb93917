"""sfmba -- MI355X-native bundle adjustment behind the reference's least_squares call.

Public surface mirrors /root/reference/sfm_lite/bundle_adjustment.py and the scipy call of
/root/reference/sfm_lite/sfm.py:266-268.  Requires libsfmba.so (HIP, gfx950); no CPU fallback.
"""
from .api import (TERMINATION_MESSAGES, apply_bundle_adjustment, compute_residuals,
                  create_sparsity_matrix, get_backend, least_squares, pack_cameras_points,
                  project_points, unpack_cameras_points)
from .backend import (Backend, BackendError, Covariance, DescriptorMatches, EssentialEstimate, FundamentalEstimate, HomographyEstimate, RelativePose, ReprojectionStats, Resection,
                      RobustResection, RobustTriangulation, SimilarityEstimate, SubProblem, Tracks, Triangulation, ViewPlan, check_plan_inputs,
                      check_similarity_inputs, check_track_inputs)
from .bal import read_bal, write_bal
from .extras import (FM_RANSAC, RANSAC, DMatch, Reconstruction, align_reconstruction, apply_similarity, build_tracks, calc_reproj_error, covariance, find_essential_mat, find_fundamental_mat, find_homography, knn_match, load_calibration_data,
                     load_problem, match_descriptors, match_features, estimate_similarity, merge_reconstructions,
                     prune_problem, reconstruct, recover_pose, refine_reconstruction, reproj_error, reprojection_stats, resect_cameras,
                     resect_cameras_ransac, save_problem, select_initial_pair, solve_pnp, solve_pnp_ransac, total_mean_reproj_error, triangulate_points,
                     triangulate_tracks, triangulate_tracks_ransac)
from .synthetic import (BAProblem, K_SCEAUX, drop_observations, growing_reconstruction, make_config,
                        make_problem, make_ring_problem)

__all__ = ["TERMINATION_MESSAGES", "apply_bundle_adjustment", "compute_residuals",
           "create_sparsity_matrix", "get_backend", "least_squares", "pack_cameras_points",
           "project_points", "unpack_cameras_points", "Backend", "BackendError", "BAProblem",
           "K_SCEAUX", "drop_observations", "growing_reconstruction", "make_config", "make_problem", "make_ring_problem",
           "calc_reproj_error", "load_calibration_data",
           "load_problem", "reproj_error", "save_problem", "read_bal", "write_bal",
           "ReprojectionStats", "reprojection_stats", "total_mean_reproj_error", "prune_problem", "refine_reconstruction",
           "Triangulation", "triangulate_tracks", "triangulate_points",
           "RobustTriangulation", "triangulate_tracks_ransac",
           "Resection", "resect_cameras", "solve_pnp",
           "RobustResection", "resect_cameras_ransac", "solve_pnp_ransac",
           "FundamentalEstimate", "RelativePose", "FM_RANSAC", "find_fundamental_mat", "recover_pose", "select_initial_pair",
           "HomographyEstimate", "RANSAC", "find_homography",
           "EssentialEstimate", "find_essential_mat",
           "DescriptorMatches", "DMatch", "knn_match", "match_descriptors", "match_features",
           "Tracks", "build_tracks", "check_track_inputs",
           "ViewPlan", "SubProblem", "check_plan_inputs", "Reconstruction", "reconstruct",
           "Covariance", "covariance",
           "SimilarityEstimate", "check_similarity_inputs", "estimate_similarity", "apply_similarity", "align_reconstruction",
           "merge_reconstructions"]
