"""Training-set extraction: Final_Project/scripts/extract.py with the reference's names.  ``read_label`` and the frame transforms run
on the host in the arithmetic include/pcr.h writes down; what the reference does once per label -- an Open3D radius query, three BLAS
calls, ``np.unique`` and a Python ``max`` -- is ONE launch for all the labels of a frame over the grouped rows of an ``ObjectBatch``
(``ObjectBatch.match_labels``, include/pcr.h "label match").  ``process_sample`` is the loop body of extract.py:506-599 on arrays.

Deviations from the reference, both of order only:
  * the rows of an extracted object come in ascending caller row, not in Open3D's ascending distance from the label's centre;
  * the centre of an object is the object sum of include/pcr.h over its selected rows, not ``.mean(axis=0)`` of the rows in distance
    order (the two differ by summation order: some 1e-14 m on full binary64 coordinates, nothing on float32-rounded ones).
And one of substance: a row DBSCAN calls noise (id -1) belongs to no object of an ``ObjectBatch``, so it is neither counted in ``k`` nor
can -1 be the chosen id, which the reference's ``np.unique`` would allow; the ``misc`` draw still treats -1 as the reference does.
Parity with Open3D's segmentation stays unpinned, as detection.py says; so does what Open3D / FLANN do with a row exactly on a
label's sphere -- here it is inside.
"""
from __future__ import annotations

import os
from random import sample

import numpy as np

from . import _lib as L
from .detection import KITTI_COLUMNS, _cloud_of, segment_ground_and_objects, transform_to_cam
from .objects import ObjectBatch, _ids

__all__ = ["read_label", "transform_from_cam_to_velo", "transform_from_velo_to_obj", "filter_by_bouding_box", "get_object_category", "init_label",
           "add_label", "get_object_pcd_df", "label_records", "match_labels", "process_sample", "LABEL_COLUMNS"]

LABEL_COLUMNS = KITTI_COLUMNS[:-1]   # a label_2 row: the detector's columns without the score


# ------------------------------------------------------------------ the host functions, elementwise in binary64
def transform_from_cam_to_velo(X_cam, param):
    """extract.py:86-114 -> (n,3): w_i = (R0[0][i]*X_0 + R0[1][i]*X_1) + R0[2][i]*X_2 (R0_rect.T . X), d = w - t,
    v_i = (R[0][i]*d_0 + R[1][i]*d_1) + R[2][i]*d_2 (R_velo_to_cam.T . d)."""
    X = np.asarray(X_cam, dtype=np.float64).reshape(-1, 3)
    R0, T = np.asarray(param["R0_rect"], dtype=np.float64), np.asarray(param["Tr_velo_to_cam"], dtype=np.float64)
    w = [(R0[0, i] * X[:, 0] + R0[1, i] * X[:, 1]) + R0[2, i] * X[:, 2] for i in range(3)]
    d = [w[i] - T[i, 3] for i in range(3)]
    return np.stack([(T[0, i] * d[0] + T[1, i] * d[1]) + T[2, i] * d[2] for i in range(3)], axis=1)


def transform_from_velo_to_obj(X_velo, param, t_obj_to_cam, ry):
    """extract.py:116-164 -> (n,3): ``transform_to_cam``, e = X - t_obj_to_cam, then R_obj_to_cam.T . e without its exact-zero terms:
    (cos*e_0 - sin*e_2, e_1, sin*e_0 + cos*e_2) -- the kernel's xo, yo before the height bias, zo."""
    X = transform_to_cam(X_velo, param)
    t = np.asarray(t_obj_to_cam, dtype=np.float64).reshape(3)
    e0, e1, e2 = X[:, 0] - t[0], X[:, 1] - t[1], X[:, 2] - t[2]
    cs, sn = np.cos(np.float64(ry)), np.sin(np.float64(ry))
    return np.stack([cs * e0 - sn * e2, e1, sn * e0 + cs * e2], axis=1)


def filter_by_bouding_box(X, labels, dims):
    """extract.py:166-201 (the reference's spelling) -> the id with the most rows inside ``-dims/2 <= X <= dims/2`` (both faces
    inclusive), the lowest such id on a tie; None when no row is inside."""
    X, labels, dims = np.asarray(X, dtype=np.float64), np.asarray(labels), np.asarray(dims, dtype=np.float64)
    idx_obj = np.all(np.logical_and(X >= -dims / 2, X <= dims / 2), axis=1)
    if idx_obj.sum() == 0:
        return None
    ids, counts = np.unique(labels[idx_obj], return_counts=True)
    object_id, _ = max(zip(ids, counts), key=lambda x: x[1])
    return object_id


def read_label(filepath, param):
    """extract.py:203-262 -> the reference's DataFrame: the 15 KITTI columns, rows with a negative dimension dropped, then ``vx, vy,
    vz`` (the centre in the Velodyne frame, ``vz`` with ``+ height/2``) and ``radius = ||0.5*(height, width, length)||``."""
    import pandas as pd   # lazily: importing the package does not import pandas

    df_label = pd.read_csv(filepath, sep=" ", header=None)
    df_label.columns = LABEL_COLUMNS
    condition = (df_label["height"] >= 0.0) & (df_label["width"] >= 0.0) & (df_label["length"] >= 0.0)
    df_label = df_label.loc[condition, df_label.columns].copy()
    centers_velo = transform_from_cam_to_velo(df_label[["cx", "cy", "cz"]].values, param)
    df_label["vx"], df_label["vy"], df_label["vz"] = centers_velo[:, 0], centers_velo[:, 1], centers_velo[:, 2]
    df_label["vz"] += df_label["height"] / 2
    hwl = df_label[["height", "width", "length"]].values.astype(np.float64)
    df_label["radius"] = [np.linalg.norm(0.5 * row) for row in hwl]
    return df_label


def init_label():
    """extract.py:264-287."""
    return {"type": [], "truncated": [], "occluded": [], "vx": [], "vy": [], "vz": [], "num_measurements": [], "height": [], "width": [], "length": [],
            "ry": []}


def add_label(dataset_label, category, label, N, center):
    """extract.py:289-336: `label` a row of read_label's frame, or None for an object without a KITTI label."""
    d = dataset_label[category]
    if label is None:
        d["type"].append("Unknown")
        d["truncated"].append(-1)
        d["occluded"].append(-1)
        d["height"].append(-1)
        d["width"].append(-1)
        d["length"].append(-1)
        d["ry"].append(-10)
    else:
        for key in ("type", "truncated", "occluded", "height", "width", "length", "ry"):
            d[key].append(label[key])
    d["num_measurements"].append(N)
    vx, vy, vz = center
    d["vx"].append(vx)
    d["vy"].append(vy)
    d["vz"].append(vz)


def get_object_pcd_df(pcd, idx, N):
    """extract.py:339-362 -> the (N,6) frame ``vx vy vz nx ny nz`` of the rows `idx` of an object with ``.points`` and ``.normals``."""
    import pandas as pd

    data = np.hstack((np.asarray(pcd.points, dtype=np.float64)[idx], np.asarray(pcd.normals, dtype=np.float64)[idx]))
    return pd.DataFrame(data=data, index=np.arange(N), columns=["vx", "vy", "vz", "nx", "ny", "nz"])


def get_object_category(object_type):
    """extract.py:364-387."""
    category = "vehicle"
    if object_type is None or object_type == "Misc" or object_type == "DontCare":
        category = "misc"
    elif object_type == "Pedestrian" or object_type == "Person_sitting":
        category = "pedestrian"
    elif object_type == "Cyclist":
        category = "cyclist"
    return category


# ------------------------------------------------------------------ the match on the device
def label_records(df_label):
    """read_label's frame -> the (L,16) records of include/pcr.h: vx, vy, vz, radius, cx, cy, cz, cos(ry), sin(ry), length, height,
    width, four zeros."""
    rec = np.zeros((len(df_label), L.PCR_LABEL_DOUBLES), dtype=np.float64)
    if len(df_label):
        rec[:, 0:4] = df_label[["vx", "vy", "vz", "radius"]].values
        rec[:, 4:7] = df_label[["cx", "cy", "cz"]].values
        ry = df_label["ry"].values.astype(np.float64)
        rec[:, 7], rec[:, 8] = np.cos(ry), np.sin(ry)
        rec[:, 9:12] = df_label[["length", "height", "width"]].values
    return rec


def match_labels(segmented_objects, object_ids, df_label, param, ctx=None):
    """The loop of extract.py:514-552 for every row of `df_label` (read_label's frame) in one device call -> dict, one entry per
    label: ``k`` rows in the label's sphere, ``object_id`` the segmented object with the most rows in the label's box (-1: none),
    ``votes`` its rows in the box, ``count`` its rows in the sphere -- the extracted sample --, ``center`` (L,3) their centre,
    ``positions`` their places within the object (ascending caller row), ``rows`` their caller rows.  `segmented_objects`: what
    ``segment_ground_and_objects`` returns (its device cloud is reused), a DeviceCloud or an (n,3) array."""
    ids = _ids(object_ids)
    cloud, owned = _cloud_of(segmented_objects, ctx)
    batch = None
    try:
        batch = ObjectBatch(cloud, ids, ctx=ctx)
        return batch.match_labels(param, label_records(df_label))
    finally:
        if batch is not None:
            batch.free()
        if owned:
            cloud.free()


def process_sample(point_cloud, param, df_label, dataset_label, output_dir=None, *, samples=None, ctx=None):
    """extract.py:506-599 on arrays: segment the scan, match every label in one call, and for every label that found an object add
    its entry to ``dataset_label[category]`` (``init_label`` containers) and emit the (N,6) frame ``vx vy vz nx ny nz`` of the
    object's in-sphere rows; then up to three objects no label chose, drawn by ``random.sample``, go to ``misc`` with all their rows
    (the reference raises when fewer than three are left; here ``min(3, unidentified)`` are drawn).  With `output_dir` the frames are
    written as ``<output_dir>/<category>/NNNNNN.txt`` (NNNNNN the running count of the category, ``index=False, header=None``) and
    the list of paths is returned; without it the list of ``(category, index, frame)``.  `samples`: the RANSAC triples of
    ``segment_ground_and_objects``.  Rows come in ascending caller row and the centre in the object-sum order (module docstring)."""
    _, objects, object_ids = segment_ground_and_objects(point_cloud, samples=samples, ctx=ctx)
    out = []

    def emit(category, frame):
        dataset_index = len(dataset_label[category]["type"])
        if output_dir is None:
            out.append((category, dataset_index, frame))
            return
        os.makedirs(os.path.join(output_dir, category), exist_ok=True)
        path = os.path.join(output_dir, category, f"{dataset_index:06d}.txt")
        frame.to_csv(path, index=False, header=None)
        out.append(path)

    try:
        identified = set()
        if len(object_ids) and object_ids.max() >= 0 and len(df_label):
            m = match_labels(objects, object_ids, df_label, param, ctx=ctx)
            for i, (_, label) in enumerate(df_label.iterrows()):
                object_id_ = int(m["object_id"][i])
                if object_id_ < 0:
                    continue
                identified.add(object_id_)
                idx_object = m["rows"][i]
                N = len(idx_object)
                category = get_object_category(label["type"])
                add_label(dataset_label, category, label, N, m["center"][i])
                emit(category, get_object_pcd_df(objects, idx_object, N))
        candidates = [i for i in np.unique(object_ids) if i not in identified]   # (the noise id -1 among them, as in the reference)
        for object_id_ in sample(candidates, min(3, len(candidates))):
            idx_object = object_ids == object_id_
            N = idx_object.sum()
            category = get_object_category(None)
            center = np.asarray(objects.points, dtype=np.float64)[idx_object].mean(axis=0)
            add_label(dataset_label, category, None, N, center)
            emit(category, get_object_pcd_df(objects, idx_object, N))
        return out
    finally:
        objects.free()
