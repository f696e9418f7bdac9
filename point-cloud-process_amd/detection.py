"""Both ends of the detector of Final_Project/scripts/detect.py:414-474 around ``objects.preprocess`` / ``objects.predict``, with the
reference's names: ``segment_ground_and_objects`` (extract.py:389-470) turns a Velodyne scan into object points and ids,
``to_kitti_eval_format`` (detect.py:56-194) turns the predictions into KITTI label rows, ``detect`` is the whole pass on arrays.

The per-object numbers of a label row -- pixel box, camera-frame centre, PCA heading on the x-z plane, extents in the heading-aligned
frame -- come from ONE launch over the grouped rows (``ObjectBatch.kitti_boxes``, include/pcr.h "KITTI boxes") instead of one mask,
three BLAS calls, a LAPACK ``eig`` and an Open3D box per object.  ``transform_to_cam``, ``transform_to_pixel`` and
``get_orientation_in_camera_frame`` are the array-level counterparts on the host, in the arithmetic the header writes down.

``segment_ground_and_objects`` composes ops the library already has (hybrid normals, the RANSAC plane of
``pcr_ground_segmentation``, DBSCAN).  Parity with Open3D's ``segment_plane`` / ``cluster_dbscan`` is UNPINNED, as for the global
initialisation: Open3D draws its triples from its own generator, refits the winning plane by least squares, and hands border points
to clusters by its own rule; here the plane is the best sampled triple's and the clustering is dbscan.py's.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .clustering import _run as _ground_run
from .dbscan import DBSCAN
from .device import DeviceCloud, default_context, points_of
from .global_registration import estimate_normals_hybrid
from .objects import ObjectBatch, _as_cloud, _ids, predict, preprocess_device

__all__ = ["read_calib", "transform_to_cam", "transform_to_pixel", "get_orientation_in_camera_frame", "object_boxes", "to_kitti_eval_format",
           "get_bounding_boxes", "segment_ground_and_objects", "detect", "SegmentedObjects", "LDS_ROWS"]

LDS_ROWS = L.PCR_KITTI_LDS_ROWS   # objects of at most this many rows keep their camera-frame rows on chip (include/pcr.h)

KITTI_COLUMNS = ["type", "truncated", "occluded", "alpha", "left", "top", "right", "bottom", "height", "width", "length", "cx", "cy", "cz", "ry", "score"]
KITTI_TYPE = {"vehicle": "Car", "pedestrian": "Pedestrian", "cyclist": "Cyclist", "misc": "Misc"}   # detect.py:84-89
_DIMENSION = {"P0": (3, 4), "P1": (3, 4), "P2": (3, 4), "P3": (3, 4), "R0_rect": (3, 3), "Tr_velo_to_cam": (3, 4), "Tr_imu_to_velo": (3, 4)}
# detect.py:218-225: pedestrian red, cyclist blue, vehicle green
_COLOR = {"pedestrian": np.asarray([0.5, 0.0, 0.0]), "cyclist": np.asarray([0.0, 0.0, 0.5]), "vehicle": np.asarray([0.0, 0.5, 0.0])}


def read_calib(filepath):
    """extract.py:49-84: one ``name: v v v ...`` line per matrix -> dict of arrays (P0..P3, Tr_* 3x4; R0_rect 3x3)."""
    param = {}
    with open(filepath, "rt") as f:
        for line in f.read().strip().split("\n"):
            name, value = tuple(line.split(":"))
            param[name] = np.asarray([float(v) for v in value.strip().split()]).reshape(_DIMENSION[name])
    return param


# ------------------------------------------------------------------ the arithmetic of include/pcr.h on the host
def transform_to_cam(X_velo, param):
    """transform_coords_utils.py:4-32 -> (n,3): u_i = ((T[i][0]*x + T[i][1]*y) + T[i][2]*z) + T[i][3], then
    X_i = (R0[i][0]*u_0 + R0[i][1]*u_1) + R0[i][2]*u_2, elementwise in binary64."""
    P = np.asarray(X_velo, dtype=np.float64).reshape(-1, 3)
    T, R0 = np.asarray(param["Tr_velo_to_cam"], dtype=np.float64), np.asarray(param["R0_rect"], dtype=np.float64)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    u = [((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3)]
    return np.stack([(R0[i, 0] * u[0] + R0[i, 1] * u[1]) + R0[i, 2] * u[2] for i in range(3)], axis=1)


def transform_to_pixel(X_cam, param):
    """transform_coords_utils.py:34-59 -> (n,2): q_i = ((P[i][0]*X_0 + P[i][1]*X_1) + P[i][2]*X_2) + P[i][3], (q_0/q_2, q_1/q_2)."""
    X = np.asarray(X_cam, dtype=np.float64).reshape(-1, 3)
    K = np.asarray(param["P2"], dtype=np.float64)
    q = [((K[i, 0] * X[:, 0] + K[i, 1] * X[:, 1]) + K[i, 2] * X[:, 2]) + K[i, 3] for i in range(3)]
    return np.stack([q[0] / q[2], q[1] / q[2]], axis=1)


def _object_sum(v):
    """The object sum of include/pcr.h: 64 partial sums over rows l, l + 64, ..., then p_l += p_{l+s} for l < s, s = 32 .. 1."""
    v = np.asarray(v, dtype=np.float64)
    p = np.zeros(64)
    for chunk in np.concatenate([v, np.zeros(-len(v) % 64)]).reshape(-1, 64):
        p = p + chunk
    s = 32
    while s >= 1:
        p[:s] = p[:s] + p[s:2 * s]
        s //= 2
    return p[0]


def _direction(a, b, c):
    cs, sn = C.c_double(), C.c_double()
    L.check(L.lib().pcr_kitti_direction(float(a), float(b), float(c), C.byref(cs), C.byref(sn)))
    return cs.value, sn.value


def get_orientation_in_camera_frame(X_cam_centered):
    """detect.py:37-54 -> yaw: the x-z moments a, b, c of the centred rows (object sums, divided by n), the direction rule of
    pcr_kitti_direction in place of ``np.linalg.eig``, then ``arctan2(sn, cs)``."""
    d = np.asarray(X_cam_centered, dtype=np.float64).reshape(-1, 3)
    n = np.float64(len(d))
    a, b, c = _object_sum(d[:, 0] * d[:, 0]) / n, _object_sum(d[:, 0] * d[:, 2]) / n, _object_sum(d[:, 2] * d[:, 2]) / n
    cs, sn = _direction(a, b, c)
    return np.arctan2(sn, cs)


# ------------------------------------------------------------------ per-object boxes
def _cloud_of(segmented_objects, ctx):
    """-> (DeviceCloud, owned): the device copy an object of segment_ground_and_objects carries, or what objects._as_cloud makes."""
    cloud = getattr(segmented_objects, "cloud", None)
    if isinstance(cloud, DeviceCloud) and cloud._h:
        return cloud, False
    return _as_cloud(segmented_objects, ctx)


def _boxes(segmented_objects, object_ids, param, ctx, wanted=None):
    """One kitti_boxes call for all objects -> (k, 16); `wanted`: the object ids to compute (the others stay NaN)."""
    ids = _ids(object_ids)
    cloud, owned = _cloud_of(segmented_objects, ctx)
    batch = None
    try:
        batch = ObjectBatch(cloud, ids, ctx=ctx)
        keep = None
        if wanted is not None:
            keep = np.zeros(batch.n_objects, dtype=np.uint8)
            for o in wanted:
                if not 0 <= int(o) < batch.n_objects:
                    raise ValueError(f"object id {o} has no rows")   # (the reference takes min() of an empty selection)
                keep[int(o)] = 1
        return batch.kitti_boxes(param, keep)
    finally:
        if batch is not None:
            batch.free()
        if owned:
            cloud.free()


def object_boxes(segmented_objects, object_ids, param, ctx=None):
    """The numbers of detect.py:106-163 for every object id 0 .. max(object_ids) -> dict of arrays: ``left, top, right, bottom``
    (pixel box), ``height, width, length`` (extents along y, x, z of the heading-aligned object frame), ``center`` (k,3) in the
    rectified camera frame, ``ry`` = arctan2 of the heading direction, ``count`` int64.  An id without rows: NaN, count 0.
    `segmented_objects`: a DeviceCloud, an (n,3) array or an object with ``.points``."""
    b = _boxes(segmented_objects, object_ids, param, ctx)
    out = {name: b[:, i].copy() for i, name in enumerate(("left", "top", "right", "bottom", "height", "width", "length"))}
    out["center"] = b[:, 7:10].copy()
    out["ry"] = np.arctan2(b[:, 11], b[:, 10])
    out["count"] = b[:, 15].astype(np.int64)
    return out


def to_kitti_eval_format(segmented_objects, object_ids, param, predictions, decoder):
    """detect.py:56-194 -> the reference's ``pandas.DataFrame``: one row per predicted object whose class is not ``'misc'``, in the
    order of `predictions` (``{class_id: {object_id: confidence}}``); 16 columns ``type truncated occluded alpha left top right
    bottom height width length cx cy cz ry score``, every number as ``f'{x:.2f}'``, truncated = occluded = -1, alpha = -10,
    score = 100 * confidence.  All objects go through one device call."""
    import pandas as pd   # lazily: importing the package does not import pandas

    fmt = lambda x: f"{x:.2f}"   # noqa: E731  (detect.py:83)
    rows = [(KITTI_TYPE[decoder[class_id]], object_id, predictions[class_id][object_id])
            for class_id in predictions if decoder[class_id] != "misc" for object_id in predictions[class_id]]
    label = {k: [] for k in ("type", "left", "top", "right", "bottom", "height", "width", "length", "cx", "cy", "cz", "ry", "score")}
    if rows:
        b = _boxes(segmented_objects, object_ids, param, None, wanted=[o for _, o, _ in rows])
        for name, object_id, confidence in rows:
            r = b[int(object_id)]
            if not r[15] > 0:
                raise ValueError(f"object id {object_id} has no rows")
            label["type"].append(name)
            for key, v in zip(("left", "top", "right", "bottom", "height", "width", "length", "cx", "cy", "cz"), r[:10]):
                label[key].append(fmt(v))
            label["ry"].append(fmt(np.arctan2(r[11], r[10])))
            label["score"].append(fmt(100.0 * confidence))
    label = pd.DataFrame.from_dict(label)
    label["truncated"] = -1
    label["occluded"] = -1
    label["alpha"] = -10   # (AOS is not evaluated)
    return label[KITTI_COLUMNS]


def get_bounding_boxes(segmented_objects, object_ids, predictions, ind2label):
    """detect.py:197-255 without Open3D: a list of ``(min_bound, max_bound, color)`` per predicted object whose class is not
    ``'misc'``, in the order of `predictions`; the bounds are the axis-aligned box of ``ObjectBatch.stats()``, the colour
    ``class_color + (1 - confidence) * class_color`` (pedestrian red, cyclist blue, vehicle green)."""
    ids = _ids(object_ids)
    cloud, owned = _cloud_of(segmented_objects, None)
    batch = None
    try:
        batch = ObjectBatch(cloud, ids)
        st = batch.stats()
    finally:
        if batch is not None:
            batch.free()
        if owned:
            cloud.free()
    bounding_boxes = []
    for class_id in predictions:
        class_name = ind2label[class_id]
        if class_name == "misc":
            continue
        class_color = _COLOR[class_name]
        for object_id in predictions[class_id]:
            confidence = predictions[class_id][object_id]
            o = int(object_id)
            bounding_boxes.append((st["min_bound"][o].copy(), st["max_bound"][o].copy(), tuple(class_color + (1.0 - confidence) * class_color)))
    return bounding_boxes


# ------------------------------------------------------------------ the front end
class SegmentedObjects:
    """What the reference keeps in an Open3D cloud: ``points`` (n,3) and ``normals`` (n,3) on the host, ``cloud`` the same rows on the
    device, ``ground_model`` (4,) = (normal, d) of the plane normal . p + d = 0."""

    def __init__(self, points, normals, cloud, ground_model):
        self.points, self.normals, self.cloud, self.ground_model = points, normals, cloud, ground_model

    def __len__(self):
        return len(self.points)

    def free(self):
        if self.cloud is not None:
            self.cloud.free()


def segment_ground_and_objects(point_cloud, *, samples=None, ctx=None):
    """extract.py:389-470 on an (N,3+) array -> ``(ground_points, objects, labels)``.

    Hybrid normals (radius 5.0, max_nn 9, unoriented); the rows with ``|n_z| > cos(pi/6)`` go to the RANSAC plane of
    ``pcr_ground_segmentation`` (tau 0.30, 1000 trials, ratio 1.0: the early break cannot fire, every trial counts);
    ``ground_points`` are that subset's inliers.  With the plane ``(normal, -normal . point)`` the objects are the rows of the whole
    cloud with ``|P . n + d| > 0.30``, ``1.95 <= x <= 80`` and ``-30 <= y <= 30``; they are uploaded once and clustered by
    ``DBSCAN(0.60, 3)``.  ``objects`` is a SegmentedObjects: ``preprocess_device(objects.cloud, labels, config,
    normals=objects.normals)`` and ``object_boxes(objects, ...)`` use its device copy.

    `samples`: (n_trials, 3) integers, the triples to try; each is taken modulo the size of the normal-filtered subset, which a
    caller cannot know beforehand.  Without it the triples are drawn as ``clustering._draw`` does, from ``np.random``.

    Parity with Open3D's ``segment_plane`` / ``cluster_dbscan`` is unpinned: Open3D uses its own generator, refits the best plane by
    least squares and has its own border-point rule."""
    ctx = ctx or default_context()
    pc = np.ascontiguousarray(points_of(point_cloud)[:, :3])
    if pc.shape[0] == 0:
        raise L.PcrError(L.PCR_E_EMPTY)
    full = DeviceCloud.upload(pc, ctx)
    try:
        normals = estimate_normals_hybrid(full, 5.0, 9, orient=False, ctx=ctx)
    finally:
        full.free()
    idx_downsampled = np.abs(normals[:, 2]) > np.cos(np.pi / 6)
    subset = np.ascontiguousarray(pc[idx_downsampled])
    if subset.shape[0] < 3:
        raise ValueError("segment_ground_and_objects: fewer than three rows have a near-vertical normal, no ground plane to fit")
    if samples is not None:
        samples = np.asarray(samples, dtype=np.int64) % subset.shape[0]
    sub = DeviceCloud.upload(subset, ctx)
    try:
        _, info = _ground_run(sub,samples, 0.30, 1000, 1.0, want_cloud=False, want_rows=False, want_mask=True)
    finally:
        sub.free()
    ground_points = subset[info["inlier_mask"]]
    normal = info["normal"]
    ground_model = np.append(normal, -np.dot(normal, info["point"]))
    P = pc.astype(np.float64)
    distance_to_ground = np.abs(np.dot(P, ground_model[:3]) + ground_model[3])
    idx = np.logical_and.reduce([distance_to_ground > 0.30, pc[:, 0] >= 1.95, pc[:, 0] <= 80.00, pc[:, 1] >= -30.00, pc[:, 1] <= +30.00])
    kept = np.ascontiguousarray(pc[idx])
    if kept.shape[0] == 0:
        return ground_points, SegmentedObjects(kept, normals[idx], None, ground_model), np.empty(0, dtype=np.int32)
    cloud = DeviceCloud.upload(kept, ctx)
    clus = DBSCAN(0.60, 3, ctx=ctx)
    clus.fit(cloud)
    return ground_points, SegmentedObjects(kept, np.ascontiguousarray(normals[idx]), cloud, ground_model), clus.predict()


def detect(model, point_cloud, param, config, ind2label, *, samples=None, ctx=None):
    """detect.py:424-473 on arrays instead of paths -> the label DataFrame: segment, ``preprocess_device``, ``predict``,
    ``to_kitti_eval_format``.  `config`: ``max_radius_distance``, ``num_sample_points``, ``batch_size``, ``num_classes``.  Writing the
    file is the caller's ``label.to_csv(path, sep=' ', header=False, index=False)``."""
    _, objects, object_ids = segment_ground_and_objects(point_cloud, samples=samples, ctx=ctx)
    try:
        if len(object_ids) == 0 or object_ids.max() < 0:
            predictions = {class_id: {} for class_id in range(int(config["num_classes"]))}
        else:
            X, ids, N = preprocess_device(objects.cloud, object_ids, config, ctx, normals=objects.normals)
            predictions = predict(X, ids, N, model, config)
        return to_kitti_eval_format(objects, object_ids, param, predictions, ind2label)
    finally:
        objects.free()
