"""ctypes binding of libpcr.so (the C ABI declared in include/pcr.h).

There is no CPU fallback: if the HIP library is missing or no AMD GPU is
present, every compute entry point raises.  Only symbol loading works on a
GPU-less host (that is what the ``-m "not gpu"`` tests check).
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PCR_LIB_PATH") or os.path.join(_HERE, "libpcr.so")  # override: A/B builds only

PCR_OK = 0
PCR_E_TOO_FEW_ASSOC = 1
PCR_E_INVALID = -1
PCR_E_EMPTY = -2
PCR_E_NOMEM = -3
PCR_E_HIP = -4
PCR_E_NO_DEVICE = -5
PCR_E_UNSUPPORTED = -6
PCR_E_TOO_MANY_ITERS = -7
PCR_E_SINGULAR = -8

PCR_INDEX_GRID = 0
PCR_INDEX_BRUTE = 1
PCR_ICP_COMPAT_MAIN = 0
PCR_ICP_TOTAL = 1
PCR_RMETRIC_FROBENIUS = 0
PCR_RMETRIC_GEODESIC = 1
PCR_ICP_MAX_LOG = 256
PCR_GMM_MAX_K = 32
PCR_KMEANS_MAX_K = 32
PCR_SPECTRAL_MAX_K = 8
PCR_SPECTRAL_MAX_NNK = 15
PCR_OBJECTS_TILE = 128
PCR_KITTI_BOX_DOUBLES = 16
PCR_KITTI_LDS_ROWS = 512
PCR_LABEL_DOUBLES = 16
PCR_LABEL_RESULT_DOUBLES = 8
PCR_KITTI_EVAL_MAX_DET = 256
PCR_KITTI_EVAL_MAX_GT = 128
PCR_KITTI_EVAL_SAMPLES = 41
PCR_KITTI_ROW_DOUBLES = 16


class IcpParams(C.Structure):
    _fields_ = [
        ("max_iter", C.c_int32),
        ("r_thres", C.c_double),
        ("t_thres", C.c_double),
        ("max_d2", C.c_double),
        ("mode", C.c_int32),
        ("r_metric", C.c_int32),
        ("min_iter", C.c_int32),
        ("reserved", C.c_int32),
    ]


class RansacParams(C.Structure):
    _fields_ = [
        ("max_iteration", C.c_int32),
        ("check_distance", C.c_int32),
        ("confidence", C.c_double),
        ("max_distance", C.c_double),
        ("edge_similarity", C.c_double),
        ("seed", C.c_uint64),
        ("reserved", C.c_double * 4),
    ]


class RansacResult(C.Structure):
    _fields_ = [
        ("T", C.c_double * 16),
        ("iterations", C.c_int32),
        ("n_valid", C.c_int32),
        ("best_iteration", C.c_int32),
        ("reserved_i", C.c_int32),
        ("corr_fitness", C.c_double),
        ("corr_rmse", C.c_double),
        ("reserved", C.c_double * 4),
    ]


class Pair(C.Structure):
    _fields_ = [
        ("src", C.POINTER(C.c_float)),
        ("n_src", C.c_int64),
        ("stride_src", C.c_int64),
        ("tgt", C.POINTER(C.c_float)),
        ("n_tgt", C.c_int64),
        ("stride_tgt", C.c_int64),
        ("T0", C.POINTER(C.c_double)),
    ]


class CloudRef(C.Structure):
    _fields_ = [("xyz", C.POINTER(C.c_float)), ("n", C.c_int64), ("stride", C.c_int64)]


class PairRef(C.Structure):
    _fields_ = [("src", C.c_int32), ("tgt", C.c_int32), ("T0", C.POINTER(C.c_double))]


class GlobalParams(C.Structure):
    _fields_ = [
        ("voxel_size", C.c_double),
        ("normal_radius", C.c_double),
        ("fpfh_radius", C.c_double),
        ("normal_max_nn", C.c_int32),
        ("fpfh_max_nn", C.c_int32),
        ("mutual_filter", C.c_int32),
        ("reserved_i", C.c_int32),
        ("ransac", RansacParams),
    ]


class IcpResult(C.Structure):
    _fields_ = [
        ("T", C.c_double * 16),
        ("T_total", C.c_double * 16),
        ("iters", C.c_int32),
        ("status", C.c_int32),
        ("n_assoc", C.c_int64),
        ("cost", C.c_double),
        ("mean_d2", C.c_double),
        ("r_diff", C.c_double * PCR_ICP_MAX_LOG),
        ("t_diff", C.c_double * PCR_ICP_MAX_LOG),
        ("device_ms", C.c_double),
        ("nn_kernel_ms", C.c_double),
        ("nn_launches", C.c_int32),
        ("reserved", C.c_int32),
    ]


class IcpPlaneParams(C.Structure):
    _fields_ = [
        ("max_iter", C.c_int32),
        ("reserved", C.c_int32),
        ("max_dist", C.c_double),
        ("rel_fitness", C.c_double),
        ("rel_rmse", C.c_double),
    ]


class IcpPlaneResult(C.Structure):
    _fields_ = [
        ("T", C.c_double * 16),
        ("fitness", C.c_double),
        ("inlier_rmse", C.c_double),
        ("n_corr", C.c_int64),
        ("iters", C.c_int32),
        ("status", C.c_int32),
        ("fitness_log", C.c_double * (PCR_ICP_MAX_LOG + 1)),
        ("rmse_log", C.c_double * (PCR_ICP_MAX_LOG + 1)),
        ("device_ms", C.c_double),
        ("nn_launches", C.c_int32),
        ("reserved", C.c_int32),
    ]


class GroundParams(C.Structure):
    _fields_ = [
        ("tau", C.c_double),
        ("ratio", C.c_double),
        ("n_hyp", C.c_int32),
        ("reserved_i", C.c_int32),
        ("reserved", C.c_double * 4),
    ]


class GroundResult(C.Structure):
    _fields_ = [
        ("best_hyp", C.c_int32),
        ("evaluated", C.c_int32),
        ("n_inliers", C.c_int64),
        ("n_outliers", C.c_int64),
        ("point", C.c_double * 3),
        ("normal", C.c_double * 3),
        ("reserved", C.c_double * 4),
    ]


class KittiCalib(C.Structure):
    _fields_ = [
        ("R0_rect", C.c_double * 9),
        ("Tr_velo_to_cam", C.c_double * 12),
        ("P2", C.c_double * 12),
        ("reserved", C.c_double * 4),
    ]


class KittiEvalParams(C.Structure):
    _fields_ = [("min_overlap", (C.c_double * 3) * 3), ("reserved", C.c_double * 7)]   # [metric][class]


class KittiEvalCell(C.Structure):
    _fields_ = [
        ("n_gt", C.c_int64),
        ("n_thresholds", C.c_int64),
        ("thresholds", C.c_double * PCR_KITTI_EVAL_SAMPLES),
        ("tp", C.c_int64 * PCR_KITTI_EVAL_SAMPLES),
        ("fp", C.c_int64 * PCR_KITTI_EVAL_SAMPLES),
        ("fn", C.c_int64 * PCR_KITTI_EVAL_SAMPLES),
        ("precision", C.c_double * PCR_KITTI_EVAL_SAMPLES),
        ("recall", C.c_double * PCR_KITTI_EVAL_SAMPLES),
        ("ap11", C.c_double),
        ("ap40", C.c_double),
    ]


class KittiEvalResult(C.Structure):
    _fields_ = [("cell", ((KittiEvalCell * 3) * 3) * 3)]   # [class][metric][difficulty]


class GmmParams(C.Structure):
    _fields_ = [
        ("n_clusters", C.c_int32),
        ("dim", C.c_int32),
        ("max_iter", C.c_int32),
        ("reserved_i", C.c_int32),
        ("tol", C.c_double),
        ("reserved", C.c_double * 4),
    ]


class GmmResult(C.Structure):
    _fields_ = [
        ("iters", C.c_int32),
        ("converged", C.c_int32),
        ("bad_component", C.c_int32),
        ("bad_iter", C.c_int32),
        ("nll", C.c_double),
        ("device_ms", C.c_double),
        ("passes", C.c_int32),
        ("reserved_i", C.c_int32),
        ("reserved", C.c_double * 4),
    ]


class KmeansParams(C.Structure):
    _fields_ = [
        ("n_clusters", C.c_int32),
        ("dim", C.c_int32),
        ("max_iter", C.c_int32),
        ("reserved_i", C.c_int32),
        ("tol", C.c_double),
        ("reserved", C.c_double * 4),
    ]


class KmeansResult(C.Structure):
    _fields_ = [
        ("iters", C.c_int32),
        ("converged", C.c_int32),
        ("n_empty", C.c_int32),
        ("reserved_i", C.c_int32),
        ("inertia", C.c_double),
        ("shift", C.c_double),
        ("device_ms", C.c_double),
        ("reserved", C.c_double * 4),
    ]


class SpectralParams(C.Structure):
    _fields_ = [
        ("n_clusters", C.c_int32),
        ("nnk", C.c_int32),
        ("normalized", C.c_int32),
        ("max_iter", C.c_int32),
        ("kmeans_max_iter", C.c_int32),
        ("reserved_i", C.c_int32),
        ("tol", C.c_double),
        ("kmeans_tol", C.c_double),
        ("reserved", C.c_double * 4),
    ]


class SpectralResult(C.Structure):
    _fields_ = [
        ("iters", C.c_int32),
        ("converged", C.c_int32),
        ("spmm", C.c_int32),
        ("max_degree", C.c_int32),
        ("bad_row", C.c_int32),
        ("kmeans_iters", C.c_int32),
        ("kmeans_converged", C.c_int32),
        ("n_empty", C.c_int32),
        ("n_edges", C.c_int64),
        ("eigenvalues", C.c_double * 8),
        ("residuals", C.c_double * 8),
        ("next_eigenvalue", C.c_double),
        ("inertia", C.c_double),
        ("graph_ms", C.c_double),
        ("solver_ms", C.c_double),
        ("kmeans_ms", C.c_double),
        ("reserved", C.c_double * 4),
    ]


class HarrisParams(C.Structure):
    _fields_ = [
        ("radius", C.c_double),
        ("threshold", C.c_double),
        ("nms", C.c_int32),
        ("refine", C.c_int32),
        ("reserved", C.c_double * 4),
    ]


_vp = C.c_void_p
_dp = C.POINTER(C.c_double)
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)

# name -> (restype, argtypes); one entry per PCR_API symbol of include/pcr.h
SIGNATURES = {
    "pcr_strerror": (C.c_char_p, [C.c_int]),
    "pcr_last_error": (C.c_char_p, [_vp]),
    "pcr_version": (C.c_char_p, []),
    "pcr_ctx_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "pcr_ctx_destroy": (C.c_int, [_vp]),
    "pcr_ctx_sync": (C.c_int, [_vp]),
    "pcr_ctx_device_info": (C.c_int, [_vp, C.c_char_p, C.POINTER(C.c_int), _lp]),
    "pcr_cloud_upload_f32": (C.c_int, [_vp, _fp, C.c_int64, C.c_int64, C.POINTER(_vp)]),
    "pcr_cloud_upload_f64": (C.c_int, [_vp, _dp, C.c_int64, C.c_int64, C.POINTER(_vp)]),
    "pcr_cloud_download_f64": (C.c_int, [_vp, _vp, _dp]),
    "pcr_cloud_size": (C.c_int64, [_vp]),
    "pcr_cloud_reordered": (C.c_int, [_vp]),
    "pcr_cloud_order": (C.c_int, [_vp, _vp, _lp]),
    "pcr_cloud_free": (C.c_int, [_vp, _vp]),
    "pcr_cloud_transform": (C.c_int, [_vp, _vp, _dp]),
    "pcr_cloud_prepare": (C.c_int, [_vp, _vp, _vp]),
    "pcr_index_build": (C.c_int, [_vp, _vp, C.c_int, C.c_double, C.POINTER(_vp)]),
    "pcr_index_free": (C.c_int, [_vp, _vp]),
    "pcr_index_kind": (C.c_int, [_vp]),
    "pcr_index_cell": (C.c_double, [_vp]),
    "pcr_index_size": (C.c_int64, [_vp]),
    "pcr_nn1": (C.c_int, [_vp, _vp, _vp, _dp, C.c_double, _ip, _dp]),
    "pcr_knn": (C.c_int, [_vp, _vp, _dp, C.c_int64, C.c_int, _ip, _dp]),
    "pcr_radius": (C.c_int, [_vp, _vp, _dp, C.c_int64, C.c_double, _lp, _lp, _ip, _dp]),
    "pcr_radius_small": (C.c_int, [_vp, _vp, _dp, C.c_int, C.c_double, C.c_int64, _lp, _ip, _dp]),
    "pcr_icp_default_params": (None, [C.POINTER(IcpParams)]),
    "pcr_icp": (C.c_int, [_vp, _vp, _vp, C.POINTER(IcpParams), _dp, C.POINTER(IcpResult)]),
    "pcr_index_set_normals": (C.c_int, [_vp, _vp, _dp]),
    "pcr_index_has_normals": (C.c_int, [_vp]),
    "pcr_icp_plane_default_params": (None, [C.POINTER(IcpPlaneParams)]),
    "pcr_icp_point2plane": (C.c_int, [_vp, _vp, _vp, C.POINTER(IcpPlaneParams), _dp, C.POINTER(IcpPlaneResult)]),
    "pcr_point2plane_moments": (C.c_int, [_vp, _vp, _vp, _dp, C.c_double, _dp]),
    "pcr_point2plane_solve": (C.c_int, [_dp, _dp, _dp, _dp]),
    "pcr_icp_batch": (C.c_int, [C.POINTER(_vp), C.c_int, C.POINTER(Pair), C.c_int64, C.POINTER(IcpParams), C.POINTER(IcpResult), _ip]),
    "pcr_global_default_params": (C.c_int, [C.c_double, C.POINTER(GlobalParams)]),
    "pcr_register_pairs": (C.c_int, [C.POINTER(_vp), C.c_int, C.POINTER(CloudRef), C.c_int64, C.POINTER(PairRef), C.c_int64, C.POINTER(GlobalParams),
                                     C.POINTER(IcpParams), C.POINTER(IcpResult), _ip, _dp]),
    "pcr_match_pairs_fused": (C.c_int, [_vp, _dp, _lp, C.c_int64, _ip, C.c_int64, C.c_int, _ip, _dp, _ip, _dp, _ip, _ip]),
    "pcr_icp_moments": (C.c_int, [_vp, _vp, _vp, _dp, C.c_double, _dp, _dp, _dp]),
    "pcr_procrustes": (C.c_int, [_dp, _dp, C.c_int64, _dp, _dp, _dp]),
    "pcr_homo2tq": (C.c_int, [_dp, _dp]),
    "pcr_voxel_keys": (C.c_int, [_vp, _dp, C.c_int64, C.c_double, _dp, _dp]),
    "pcr_voxel_filter": (C.c_int, [_vp, _dp, C.c_int64, C.c_double, C.c_int, C.c_uint64, _dp, _lp]),
    "pcr_voxel_filter_cloud": (C.c_int, [_vp, _vp, C.c_double, C.c_int, C.c_uint64, C.POINTER(_vp)]),
    "pcr_iss": (C.c_int, [_vp, _vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, _dp, _ip, _ip, C.POINTER(C.c_int)]),
    "pcr_harris_default_params": (None, [C.POINTER(HarrisParams)]),
    "pcr_normals_radius": (C.c_int, [_vp, _vp, C.c_double, _dp, _dp, _ip]),
    # (ctx, cloud, normals | NULL, params, response, counts, keypoints, capacity, n_keypoints, keypoint responses, refined, rounds)
    "pcr_harris3d": (C.c_int, [_vp, _vp, _dp, C.POINTER(HarrisParams), _dp, _ip, _ip, C.c_int64, _lp, _dp, _dp, _ip]),
    # (ctx, cloud, salient radius, non-max radius, gamma21, gamma32, min_neighbors, scores, counts, keypoints, capacity, n_keypoints)
    "pcr_iss_pcl": (C.c_int, [_vp, _vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, _dp, _ip, _ip, C.c_int64, _lp]),
    "pcr_sift_scales": (C.c_int, [C.c_double, C.c_int, _dp]),
    # (ctx, cloud, base scale, scales per octave, min contrast, field, dog | NULL, counts | NULL, rows, columns, capacity, n)
    "pcr_sift_octave": (C.c_int, [_vp, _vp, C.c_double, C.c_int, C.c_double, C.c_int, _dp, _ip, _ip, _ip, C.c_int64, _lp]),
    # (ctx, cloud, dog, columns, min contrast, rows, columns, capacity, n)
    "pcr_sift_extrema": (C.c_int, [_vp, _vp, _dp, C.c_int, C.c_double, _ip, _ip, C.c_int64, _lp]),
    # (ctx, cloud, min scale, octaves, scales per octave, min contrast, field, keypoints, octave | NULL, row | NULL, capacity, n, octave sizes | NULL)
    "pcr_sift": (C.c_int, [_vp, _vp, C.c_double, C.c_int, C.c_int, C.c_double, C.c_int, _dp, _ip, _ip, C.c_int64, _lp, _lp]),
    # (ctx, cloud, k, viewpoint | NULL, normals, curvature | NULL)
    "pcr_normals_knn": (C.c_int, [_vp, _vp, C.c_int, _dp, _dp, _dp]),
    # (ctx, surface, normals, keypoints, m, radius, features, counts | NULL, n_spfh | NULL)
    "pcr_fpfh_pcl": (C.c_int, [_vp, _vp, _dp, _dp, C.c_int64, C.c_double, _dp, _ip, _lp]),
    # (ctx, surface, keypoints, m, radius, frames, counts | NULL)
    "pcr_shot_lrf": (C.c_int, [_vp, _vp, _dp, C.c_int64, C.c_double, _dp, _ip]),
    # (ctx, surface, normals, keypoints, m, radius, frames_in | NULL, features, frames_out | NULL, counts | NULL)
    "pcr_shot352": (C.c_int, [_vp, _vp, _dp, _dp, C.c_int64, C.c_double, _dp, _dp, _dp, _ip]),
    "pcr_pca": (C.c_int, [_vp, _vp, _dp, _dp, _dp]),
    "pcr_normals": (C.c_int, [_vp, _vp, C.c_int, _dp, _dp, _ip]),
    "pcr_normals_hybrid": (C.c_int, [_vp, _vp, C.c_double, C.c_int, C.c_int, _dp, _dp]),
    "pcr_fpfh": (C.c_int, [_vp, _vp, _dp, C.c_double, C.c_int, _dp]),
    "pcr_fpfh_rows": (C.c_int, [_vp, _vp, _dp, C.c_double, C.c_int, _lp, C.c_int64, _dp, _lp]),
    "pcr_feature_match": (C.c_int, [_vp, _dp, C.c_int64, _dp, C.c_int64, C.c_int, _ip, _dp]),
    "pcr_ransac_default_params": (C.c_int, [C.POINTER(RansacParams)]),
    "pcr_ransac": (C.c_int, [_vp, _vp, _vp, _ip, C.c_int64, C.POINTER(RansacParams), C.POINTER(RansacResult)]),
    "pcr_preprocess": (C.c_int, [_vp, _vp, C.c_double, C.c_double, C.c_int, C.c_double, C.c_int, C.POINTER(_vp)]),
    "pcr_prep_size": (C.c_int64, [_vp]),
    "pcr_prep_cloud": (_vp, [_vp]),
    "pcr_prep_download": (C.c_int, [_vp, _vp, _dp, _dp, _dp]),
    "pcr_prep_free": (C.c_int, [_vp, _vp]),
    "pcr_global_registration": (C.c_int, [_vp, _vp, _vp, C.POINTER(RansacParams), C.c_int, C.POINTER(RansacResult)]),
    "pcr_dbscan": (C.c_int, [_vp, _vp, C.c_double, C.c_int, _ip, _ip]),
    "pcr_ground_default_params": (None, [C.POINTER(GroundParams)]),
    "pcr_ground_select": (C.c_int, [_lp, C.c_int32, C.c_int64, C.c_double, _ip, _ip]),
    "pcr_ground_segmentation": (C.c_int, [_vp, _vp, _lp, C.POINTER(GroundParams), C.POINTER(_vp), _ip, C.POINTER(C.c_uint8), _lp, C.POINTER(GroundResult)]),
    "pcr_gmm_default_params": (None, [C.POINTER(GmmParams)]),
    "pcr_gmm_fit": (C.c_int, [_vp, _vp, C.POINTER(GmmParams), _dp, _dp, _dp, _dp, _dp, C.POINTER(GmmResult)]),
    "pcr_gmm_step": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "pcr_gmm_predict": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _dp, _dp, _dp, _ip, _dp, _dp]),
    "pcr_gmm_log_density": (C.c_int, [C.c_int, _dp, _dp, _dp, C.c_double, _dp]),
    "pcr_kmeans_default_params": (None, [C.POINTER(KmeansParams)]),
    "pcr_kmeans_fit": (C.c_int, [_vp, _vp, C.POINTER(KmeansParams), _dp, _dp, _lp, _ip, _dp, _dp, C.POINTER(KmeansResult)]),
    "pcr_kmeans_step": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _dp, _dp, _lp, _dp, _dp, _dp]),
    "pcr_kmeans_predict": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _dp, _ip, _lp, _dp]),
    "pcr_cloud_download_rows": (C.c_int, [_vp, _vp, _lp, C.c_int64, _dp]),
    "pcr_spectral_default_params": (None, [C.POINTER(SpectralParams)]),
    "pcr_knn_graph": (C.c_int, [_vp, _vp, C.c_int, _lp, _ip, _dp, _ip]),
    "pcr_spectral_embed": (C.c_int, [_vp, _vp, C.POINTER(SpectralParams), _dp, C.POINTER(SpectralResult)]),
    "pcr_spectral_fit": (C.c_int, [_vp, _vp, C.POINTER(SpectralParams), _lp, _ip, _dp, _dp, _lp, C.POINTER(SpectralResult)]),
    "pcr_sym_eig_jacobi": (C.c_int, [C.c_int, _dp, _dp, _dp]),
    # PointNet++ ops: (stream, sizes..., device pointers...) -- addresses of the caller's device tensors, hence plain void*
    "pcr_pn2_furthest_point_sampling": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp]),
    "pcr_pn2_ball_query": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _vp, _vp, _vp]),
    "pcr_pn2_three_nn": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "pcr_pn2_three_interpolate": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "pcr_pn2_gather_points": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp]),
    "pcr_pn2_group_points": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp]),
    # the gradients in a fixed order: the inverse index of an index tensor (workspace size, build), then the three sums over it
    "pcr_pn2_inverse_index_bytes": (C.c_longlong, [C.c_int, C.c_int, C.c_int]),
    "pcr_pn2_inverse_index": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_longlong, _vp, _vp]),
    "pcr_pn2_gather_points_grad": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "pcr_pn2_group_points_grad": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "pcr_pn2_three_interpolate_grad": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    # (stream, b, n, m, nsample, c_feat, use_xyz, xyz, new_xyz, feats, idx, n_layers, host widths, host weight / bias pointer arrays, out, stride)
    "pcr_pn2_sa_mlp_max": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_int, C.POINTER(C.c_int),
                                     C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _vp, C.c_longlong]),
    # (stream, b, n, m, c_known, c_skip, known_feats, idx, weight, skip_feats, n_layers, host widths, host weight / bias pointer arrays, relu_last, out)
    "pcr_pn2_fp_mlp": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_int, C.POINTER(C.c_int),
                                 C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, _vp]),
    # object batches: (ctx, objects handle, host arrays...); the pack's last argument is the address of the caller's device tensor
    "pcr_objects_build": (C.c_int, [_vp, _vp, _ip, C.c_int32, C.POINTER(_vp)]),
    "pcr_objects_free": (C.c_int, [_vp, _vp]),
    "pcr_objects_offsets": (C.c_int, [_vp, _lp]),
    "pcr_objects_rows": (C.c_int, [_vp, _vp, _ip]),
    "pcr_objects_stats": (C.c_int, [_vp, _vp, _lp, _dp, _dp, _dp]),
    "pcr_objects_select": (C.c_int, [_lp, _dp, C.c_int32, C.c_int64, C.c_double, C.POINTER(C.c_uint8)]),
    "pcr_objects_weights": (C.c_int, [_vp, _vp, C.POINTER(C.c_uint8), _dp]),
    "pcr_objects_pack_f32": (C.c_int, [_vp, _vp, _dp, _ip, _lp, C.c_int64, C.c_int64, _vp]),
    # KITTI boxes: the direction rule on the host, and (ctx, objects handle, calibration, keep flags, n_objects x 16 doubles)
    "pcr_kitti_direction": (C.c_int, [C.c_double, C.c_double, C.c_double, _dp, _dp]),
    "pcr_objects_kitti_boxes": (C.c_int, [_vp, _vp, C.POINTER(KittiCalib), C.POINTER(C.c_uint8), _dp]),
    # label match: (ctx, objects handle, calibration, L x 16 label doubles, L, L x 8 result doubles, L x words ballot words or NULL, words)
    "pcr_objects_match_labels": (C.c_int, [_vp, _vp, C.POINTER(KittiCalib), _dp, C.c_int64, _dp, C.POINTER(C.c_uint64), C.c_int64]),
    # KITTI evaluation: (ctx, det rows, det_first, gt rows, gt_first, F, ...); the overlap of one pair on the host
    "pcr_kitti_eval_default_params": (None, [C.POINTER(KittiEvalParams)]),
    "pcr_kitti_box_overlap": (C.c_int, [_dp, _dp, C.c_int, C.c_int, _dp]),
    "pcr_kitti_eval_overlaps": (C.c_int, [_vp, _dp, _lp, _dp, _lp, C.c_int64, C.c_int, _dp, _dp, _dp, _lp]),
    "pcr_kitti_eval_match": (C.c_int, [_vp, _dp, _lp, _dp, _lp, C.c_int64, C.POINTER(KittiEvalParams), C.c_int, C.c_int, C.c_int, _dp, C.c_int, C.c_int,
                                       _lp, _lp, _lp, _dp, _lp]),
    "pcr_kitti_eval": (C.c_int, [_vp, _dp, _lp, _dp, _lp, C.c_int64, C.POINTER(KittiEvalParams), C.POINTER(KittiEvalResult), _dp]),
    "pcr_debug_read": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.c_int64]),
    "pcr_debug_arena": (C.c_int, [_vp, _lp]),
    "pcr_debug_fail_alloc": (C.c_int, [_vp, C.c_int]),
    # (ctx or NULL for the host build, op, n x in doubles, n, n x out doubles): include/pcr.h lists the doubles per op
    "pcr_debug_linalg": (C.c_int, [_vp, C.c_int, _dp, C.c_int64, _dp]),
    "pcr_profile_enable": (C.c_int, [_vp, C.c_int]),
    "pcr_profile_read": (C.c_int, [_vp, _dp, C.POINTER(C.c_int)]),
    "pcr_search_stats": (C.c_int, [_vp, _lp]),
    "pcr_ctx_set_shared": (C.c_int, [_vp, C.c_int]),
    "pcr_icp_pass_log": (C.c_int, [_vp, C.c_int, _dp, _dp, _lp, C.POINTER(C.c_int), _dp]),
    "pcr_timer_start": (C.c_int, [_vp]),
    "pcr_timer_stop_ms": (C.c_int, [_vp, _dp]),
}

_lib = None


class PcrError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        msg = f"libpcr status {status}"
        try:
            msg += ": " + lib().pcr_strerror(status).decode()
        except Exception:
            pass
        if detail:
            msg += f" ({detail})"
        super().__init__(msg)


def lib():
    """Load libpcr.so (built by __graft_entry__.build()).  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()'). "
            "There is no CPU fallback for the registration path."
        )
    # One HIP runtime per process: PyTorch ships its own libamdhip64 (same soname);
    # importing torch first makes libpcr.so bind to that copy instead of loading a
    # second runtime from /opt/rocm.
    if "torch" not in sys.modules and os.environ.get("PCR_NO_TORCH_PRELOAD", "0") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)  # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(status, ctx=None, soft=(PCR_E_TOO_FEW_ASSOC,)):
    if status == PCR_OK or status in soft:
        return status
    detail = ""
    if ctx is not None and status == PCR_E_HIP:
        try:
            detail = lib().pcr_last_error(ctx).decode()
        except Exception:
            pass
    raise PcrError(status, detail)


def as_f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def dptr(a):
    return a.ctypes.data_as(_dp)


def iptr(a):
    return a.ctypes.data_as(_ip)


def lptr(a):
    return a.ctypes.data_as(_lp)
