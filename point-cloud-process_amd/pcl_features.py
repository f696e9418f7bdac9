"""The PCL-rule FPFH descriptors of the reference's pybind module PCLKeypoint (PCLKeypoints/src/keypoints.cpp:112-184,272-281) on the
device, under names of their own: ``fpfh33`` (featureFPFH33), ``fpfh33_with_normal`` (featureFPFH33WithNormal) and the k-nearest
normals they rest on, ``estimate_normals_knn``.  The rules are stated in include/pcr.h (pcr_normals_knn, pcr_fpfh_pcl): keypoints are
COORDINATES searched against the cloud as search surface, the neighbourhood is the radius ball alone with no cap, the weighted sum is
normalised and nothing is added to it.  PCL itself is not used and no version of it is pinned: parity with its binary32 output is
unpinned.  ``compute_fpfh_feature`` / ``compute_fpfh_at_rows`` follow Open3D's rules and are other descriptors.

The module's second descriptor, SHOT352 (keypoints.cpp:187-235,282-291), takes the same arguments: ``shot352`` (featureSHOT352),
``shot352_with_normal`` (featureSHOT352WithNormal) and the local reference frames under them, ``shot_lrf``; rules in include/pcr.h
(pcr_shot_lrf, pcr_shot352), parity with PCL's binary32 output unpinned as well.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .device import DeviceCloud, default_context, points_of

__all__ = ["fpfh33", "fpfh33_with_normal", "estimate_normals_knn", "shot352", "shot352_with_normal", "shot_lrf"]


def _cloud(points, ctx):
    """-> (DeviceCloud, the one to free or None)."""
    if isinstance(points, DeviceCloud):
        return points, None
    c = DeviceCloud.upload(np.ascontiguousarray(points_of(points)[:, :3], dtype=np.float64), ctx)
    return c, c


def _keypoints(keypoints):
    """Any (m,>=3) array-like (a list, float32, a strided view; keypointHarris3D's (K,4) rows as they are) -> contiguous (m,3) float64."""
    kp = np.asarray(keypoints, dtype=np.float64)
    if kp.size == 0:
        return np.empty((0, 3), dtype=np.float64)
    if kp.ndim != 2 or kp.shape[1] < 3:
        raise ValueError("keypoints must be (m, >=3) coordinates")
    return np.ascontiguousarray(kp[:, :3])


def _viewpoint(viewpoint):
    return L.as_f64(np.asarray(viewpoint, dtype=np.float64).reshape(3))


def _normals_knn(ctx, cloud, k, viewpoint, want_curvature):
    out = np.empty((cloud.n, 3), dtype=np.float64)
    curv = np.empty(cloud.n, dtype=np.float64) if want_curvature else None
    vp = _viewpoint(viewpoint)
    L.check(L.lib().pcr_normals_knn(ctx.handle, cloud.handle, int(k), L.dptr(vp), L.dptr(out), L.dptr(curv) if want_curvature else None), ctx.handle,
            soft=())
    return out, curv


def _fpfh_pcl(ctx, cloud, nrm, kp, radius):
    """-> ((m,33) float64, info)"""
    m = kp.shape[0]
    out = np.empty((m, 33), dtype=np.float64)
    counts = np.empty(m, dtype=np.int32)
    n_spfh = C.c_int64(0)
    L.check(L.lib().pcr_fpfh_pcl(ctx.handle, cloud.handle, L.dptr(nrm), L.dptr(kp), m, float(radius), L.dptr(out), L.iptr(counts), C.byref(n_spfh)), ctx.handle, soft=())
    return out, {"counts": counts, "n_spfh": int(n_spfh.value), "n": int(cloud.n), "m": int(m)}


def estimate_normals_knn(points, k=10, viewpoint=(0.0, 0.0, 0.0), *, return_curvature=False, ctx=None):
    """pcl::NormalEstimation with setKSearch(k) (what featureFPFH33 runs first) -> (N,3) float64: the smallest eigenvector of the
    covariance of every row's ``k`` nearest rows (itself included, ordered by distance then row), flipped toward ``viewpoint``.
    ``return_curvature`` adds (N,) e_min / (e0 + e1 + e2).  3 <= k <= 16."""
    ctx = ctx or default_context()
    cloud, own = _cloud(points, ctx)
    try:
        out, curv = _normals_knn(ctx, cloud, k, viewpoint, return_curvature)
    finally:
        if own is not None:
            own.free()
    return (out, curv) if return_curvature else out


def fpfh33_with_normal(pointcloud, normals, keypoints, feature_radius=1.0, *, ctx=None, return_info=False):
    """featureFPFH33WithNormal (keypoints.cpp:162-184) -> float32 (m,33): the PCL-rule FPFH of the ``keypoints`` -- (m,>=3)
    coordinates, on the cloud or not -- over ``pointcloud`` as search surface with its per-row ``normals`` (N,3).  A keypoint with
    nothing within ``feature_radius``, or one that is not finite, gets 33 NaN.  ``pointcloud``: (N,>=3) array-like, an object with
    ``.points``, or a DeviceCloud.  ``return_info`` adds {"counts": (m,) int32 rows in every ball, "n_spfh": rows whose SPFH was
    computed, "n": cloud rows, "m": keypoints}."""
    ctx = ctx or default_context()
    kp = _keypoints(keypoints)
    cloud, own = _cloud(pointcloud, ctx)
    try:
        nrm = L.as_f64(np.asarray(normals, dtype=np.float64).reshape(-1, 3))
        if nrm.shape[0] != cloud.n:
            raise ValueError("normals do not match the cloud")
        out, info = _fpfh_pcl(ctx, cloud, nrm, kp, feature_radius)
    finally:
        if own is not None:
            own.free()
    out = out.astype(np.float32)
    return (out, info) if return_info else out


def fpfh33(pointcloud, keypoints, compute_normal_k=10, feature_radius=1.0, *, viewpoint=(0.0, 0.0, 0.0), ctx=None, return_info=False):
    """featureFPFH33 (keypoints.cpp:112-160) -> float32 (m,33): ``estimate_normals_knn(pointcloud, compute_normal_k, viewpoint)``, then
    ``fpfh33_with_normal`` with those normals; the cloud is uploaded once."""
    ctx = ctx or default_context()
    kp = _keypoints(keypoints)
    cloud, own = _cloud(pointcloud, ctx)
    try:
        nrm, _ = _normals_knn(ctx, cloud, compute_normal_k, viewpoint, False)
        out, info = _fpfh_pcl(ctx, cloud, nrm, kp, feature_radius)
    finally:
        if own is not None:
            own.free()
    out = out.astype(np.float32)
    return (out, info) if return_info else out


def _shot352(ctx, cloud, nrm, kp, radius, frames=None):
    """-> ((m,352) float64, info)"""
    m = kp.shape[0]
    out = np.empty((m, 352), dtype=np.float64)
    used = np.empty((m, 9), dtype=np.float64)
    counts = np.empty(m, dtype=np.int32)
    L.check(L.lib().pcr_shot352(ctx.handle, cloud.handle, L.dptr(nrm), L.dptr(kp), m, float(radius), L.dptr(frames) if frames is not None else None, L.dptr(out), L.dptr(used),
                                L.iptr(counts)), ctx.handle, soft=())
    return out, {"counts": counts, "frames": used.reshape(m, 3, 3), "n": int(cloud.n), "m": int(m)}


def shot_lrf(pointcloud, keypoints, radius=1.0, *, ctx=None, return_counts=False):
    """SHOTLocalReferenceFrameEstimation at the ``keypoints`` -- (m,>=3) coordinates, on the cloud or not -- over ``pointcloud`` as search
    surface -> (m,3,3) float64, rows x, y, z.  A ball of fewer than 5 rows, or a keypoint that is not finite: 9 NaN.  ``return_counts``
    adds the (m,) int32 rows in every ball."""
    ctx = ctx or default_context()
    kp = _keypoints(keypoints)
    cloud, own = _cloud(pointcloud, ctx)
    try:
        m = kp.shape[0]
        frames = np.empty((m, 9), dtype=np.float64)
        counts = np.empty(m, dtype=np.int32)
        L.check(L.lib().pcr_shot_lrf(ctx.handle, cloud.handle, L.dptr(kp), m, float(radius), L.dptr(frames), L.iptr(counts)), ctx.handle, soft=())
    finally:
        if own is not None:
            own.free()
    frames = frames.reshape(m, 3, 3)
    return (frames, counts) if return_counts else frames


def shot352_with_normal(pointcloud, normals, keypoints, feature_radius=1.0, *, frames=None, ctx=None, return_info=False):
    """featureSHOT352WithNormal (keypoints.cpp:214-235) -> float32 (m,352): the SHOT descriptor of the ``keypoints`` -- (m,>=3)
    coordinates, on the cloud or not -- over ``pointcloud`` as search surface with its per-row ``normals`` (N,3).  A keypoint with fewer
    than 5 rows within ``feature_radius``, one that is not finite, or one whose neighbours all lack a normal gets 352 NaN.  ``frames``
    (m,3,3) or (m,9): reference frames to use instead of the computed ones (setInputReferenceFrames).  ``return_info`` adds {"counts":
    (m,) int32 rows in every ball, "frames": (m,3,3) the frames used, "n": cloud rows, "m": keypoints}."""
    ctx = ctx or default_context()
    kp = _keypoints(keypoints)
    cloud, own = _cloud(pointcloud, ctx)
    try:
        nrm = L.as_f64(np.asarray(normals, dtype=np.float64).reshape(-1, 3))
        if nrm.shape[0] != cloud.n:
            raise ValueError("normals do not match the cloud")
        if frames is not None:
            frames = L.as_f64(np.asarray(frames, dtype=np.float64).reshape(-1, 9))
            if frames.shape[0] != kp.shape[0]:
                raise ValueError("frames do not match the keypoints")
        out, info = _shot352(ctx, cloud, nrm, kp, feature_radius, frames)
    finally:
        if own is not None:
            own.free()
    out = out.astype(np.float32)
    return (out, info) if return_info else out


def shot352(pointcloud, keypoints, compute_normal_k=10, feature_radius=1.0, *, viewpoint=(0.0, 0.0, 0.0), ctx=None, return_info=False):
    """featureSHOT352 (keypoints.cpp:187-211) -> float32 (m,352): ``estimate_normals_knn(pointcloud, compute_normal_k, viewpoint)``, then
    ``shot352_with_normal`` with those normals; the cloud is uploaded once."""
    ctx = ctx or default_context()
    kp = _keypoints(keypoints)
    cloud, own = _cloud(pointcloud, ctx)
    try:
        nrm, _ = _normals_knn(ctx, cloud, compute_normal_k, viewpoint, False)
        out, info = _shot352(ctx, cloud, nrm, kp, feature_radius)
    finally:
        if own is not None:
            own.free()
    out = out.astype(np.float32)
    return (out, info) if return_info else out
