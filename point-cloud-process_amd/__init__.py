"""MI355X-native registration hot path (ICP + nearest neighbour + voxel filter).

Drop-in for the reference's Registration/main.py, Registration/icp_template.py,
Kdtree_Octree/lesson2 and Pca_and_Voxel_filter/voxel_filter.py call surfaces,
backed by hand-written HIP kernels for gfx950 behind the C ABI in include/pcr.h.

The directory name contains a hyphen, so import it with
``importlib.import_module("point-cloud-process_amd")`` or through the
top-level alias module ``pcp_amd``.
"""
from . import _lib  # noqa: F401
from . import synthetic  # noqa: F401
from .device import Context, DeviceCloud, TargetIndex, default_context, icp_device, icp_point2plane_device  # noqa: F401
from .registration import (  # noqa: F401
    ICP,
    ICPConvergenceCriteria,
    TransformationEstimationPointToPlane,
    coarse_to_fine_icp,
    KDTreeFlann,
    PointCloud,
    copysign,
    find_associations,
    homo2tq,
    icp_point2point,
    procrustes_transformation,
    read_bin_velodyne,
    read_oxford_bin,
    read_velodyne_bin,
    refine_registration,
    registration_icp,
    rotmat2quaternion,
    write_reg_result,
)

from .voxel_filter import voxel_filter, voxel_filter_device, voxel_keys  # noqa: F401
from .result_set import DistIndex, KNNResultSet, RadiusNNResultSet  # noqa: F401
from .kdtree import kdtree_construction, kdtree_knn_search, kdtree_radius_search, knn_search_batch, radius_search_batch  # noqa: F401
from .octree import octree_construction, octree_knn_search, octree_radius_search, octree_radius_search_fast  # noqa: F401
from .iss import iss_keypoints  # noqa: F401
from .pca_normal import PCA, estimate_normals  # noqa: F401
from .global_registration import (  # noqa: F401
    Feature,
    RegistrationResult,
    compute_fpfh_at_rows,
    compute_fpfh_feature,
    estimate_normals_hybrid,
    estimate_normals_radius,
    execute_global_registration,
    find_matchings,
    prepare_dataset,
    preprocess_point_cloud,
    ransac_init,
    registration_ransac_based_on_feature_matching,
    voxel_down_sample,
)
from . import PCLKeypoint  # noqa: F401
from .PCLKeypoint import keypointHarris3D, keypointIss  # noqa: F401
from . import pcl_features  # noqa: F401
from .pcl_features import estimate_normals_knn, fpfh33, fpfh33_with_normal, shot352, shot352_with_normal, shot_lrf  # noqa: F401
from . import pcl_keypoints  # noqa: F401
from .pcl_keypoints import sift_extrema, sift_keypoints, sift_octave, sift_scales  # noqa: F401
from .dbscan import DBSCAN  # noqa: F401
from .clustering import clustering, ground_segmentation, segment_and_cluster  # noqa: F401
from . import objects  # noqa: F401
from .objects import ObjectBatch, object_stats, predict, preprocess, preprocess_device, resample_weights  # noqa: F401
from . import detection  # noqa: F401
from .detection import (  # noqa: F401
    detect,
    get_bounding_boxes,
    get_orientation_in_camera_frame,
    object_boxes,
    read_calib,
    segment_ground_and_objects,
    to_kitti_eval_format,
    transform_to_cam,
    transform_to_pixel,
)
from . import extract  # noqa: F401
from .extract import (  # noqa: F401
    add_label,
    filter_by_bouding_box,
    get_object_category,
    get_object_pcd_df,
    init_label,
    label_records,
    match_labels,
    process_sample,
    read_label,
    transform_from_cam_to_velo,
    transform_from_velo_to_obj,
)
from . import kitti_eval  # noqa: F401
from .kitti_eval import box_overlaps, evaluate_object_3d_offline, frames_from, read_label_dir, read_label_file  # noqa: F401
from .gmm import GMM  # noqa: F401
from .kmeans import K_Means  # noqa: F401
from .spectral import knn_graph, spectral_clustering, spetral_clustering  # noqa: F401
from .batch import register_batch, shard_range  # noqa: F401
from . import evaluate  # noqa: F401
from .evaluate import evaluate_rt, get_P_diff, is_registration_successful  # noqa: F401
from .drivers import read_pair_list, run_registration  # noqa: F401

__version__ = "0.1.0"

# The PointNet++ ops are torch modules and autograd functions: they come in on first use, so that importing the package does not
# import torch (see PCR_NO_TORCH_PRELOAD in _lib.py).
_POINTNET2_EXPORTS = ("pointnet2_ops", "pointnet2_utils", "pointnet2_modules", "furthest_point_sample_np", "pointnet2_models",
                      "PointNet2ClassificationSSG", "PointNet2ClassificationMSG", "PointNet2SemSegSSG", "PointNet2SemSegMSG")


def __getattr__(name):
    if name in _POINTNET2_EXPORTS:
        import importlib

        ops = importlib.import_module(__name__ + ".pointnet2_ops")
        return ops if name == "pointnet2_ops" else getattr(ops, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
