"""The XYZ keypoint detectors of the reference's pybind module PCLKeypoint (PCLKeypoints/src/keypoints.cpp:243-291) on the device:
``keypointHarris3D`` and ``keypointIss`` with the wrapper's names and defaults, by the rules stated in include/pcr.h
(pcr_harris3d, pcr_iss_pcl).  PCL itself is not used and no version of it is pinned: parity with its binary32 output is unpinned.
``iss_keypoints`` (ISS.py's detector) is another function and stays what it is.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .device import DeviceCloud, default_context, points_of

__all__ = ["keypointHarris3D", "keypointIss", "keypointHarris6D", "keypointSift", "featureFPFH33", "featureFPFH33WithNormal", "featureSHOT352",
           "featureSHOT352WithNormal"]


def _cloud(points, ctx):
    """-> (DeviceCloud, the one to free or None, host (N,3) float64 or None)."""
    if isinstance(points, DeviceCloud):
        return points, None, None
    host = np.ascontiguousarray(points_of(points)[:, :3], dtype=np.float64)
    c = DeviceCloud.upload(host, ctx)
    return c, c, host


def _positions(cloud, host, rows, ctx):
    """Positions of the caller rows `rows` (ascending): from the host array if there is one, else from the device -- the few rows of a
    keypoint list by row (4096 per call), more than a quarter of the cloud as one download."""
    if host is not None:
        return host[rows]
    if 4 * len(rows) > cloud.n:
        return cloud.download()[rows]
    out = np.empty((len(rows), 3), dtype=np.float64)
    for first in range(0, len(rows), 4096):
        out[first:first + 4096] = cloud.download_rows(rows[first:first + 4096])
    return out


def keypointHarris3D(points, radius=0.5, nms_threshold=0.001, threads=0, is_nms=False, is_refine=False, *, normals=None, return_indices=False,
                     return_details=False, ctx=None):
    """keypoints.cpp:136-160 -> float32 (K,4): x, y, z, intensity (the Harris response).  ``is_nms=False`` returns every row with its
    response; ``is_nms=True`` the rows whose response is >= ``nms_threshold`` and that no row within ``radius`` beats; ``is_refine``
    (only together with ``is_nms``) moves every kept corner onto the local intersection of the tangent planes.  ``threads`` is accepted
    and ignored.  ``points``: (N,>=3) array-like, an object with ``.points``, or a DeviceCloud.

    Keyword-only: ``normals`` (N,3) replaces the radius normals (rows without one hold NaN); ``return_indices`` adds the caller rows
    (K,) int64; ``return_details`` adds a dict with ``response`` (N,) float64, ``counts`` (N,) int32 and, when refining, ``rounds`` (K,)."""
    del threads
    ctx = ctx or default_context()
    cloud, own, host = _cloud(points, ctx)
    try:
        n = cloud.n
        p = L.HarrisParams()
        L.lib().pcr_harris_default_params(C.byref(p))
        p.radius, p.threshold, p.nms, p.refine = float(radius), float(nms_threshold), int(bool(is_nms)), int(bool(is_nms and is_refine))
        nrm = None
        if normals is not None:
            nrm = L.as_f64(np.asarray(normals, dtype=np.float64).reshape(-1, 3))
            if nrm.shape[0] != n:
                raise ValueError("normals do not match the cloud")
        resp = np.empty(n, dtype=np.float64) if (return_details or not is_nms) else None
        counts = np.empty(n, dtype=np.int32) if return_details else None
        details = {}
        if is_nms:
            # the host buffers could hold every row; the library fills (and moves over PCIe) the keypoints only
            kp = np.empty(n, dtype=np.int32)
            kresp = np.empty(n, dtype=np.float64)
            refined = np.empty((n, 3), dtype=np.float64) if p.refine else None
            rounds = np.empty(n, dtype=np.int32) if p.refine else None
            nk = C.c_int64()
            L.check(L.lib().pcr_harris3d(ctx.handle, cloud.handle, L.dptr(nrm) if nrm is not None else None, C.byref(p), L.dptr(resp) if resp is not None else None,
                                         L.iptr(counts) if counts is not None else None, L.iptr(kp), n, C.byref(nk), L.dptr(kresp),
                                         L.dptr(refined) if p.refine else None, L.iptr(rounds) if p.refine else None), ctx.handle)
            rows = kp[: nk.value].astype(np.int64)
            xyz = refined[: nk.value] if p.refine else _positions(cloud, host, rows, ctx)
            intensity = kresp[: nk.value]
            if p.refine:
                details["rounds"] = rounds[: nk.value].copy()
        else:
            L.check(L.lib().pcr_harris3d(ctx.handle, cloud.handle, L.dptr(nrm) if nrm is not None else None, C.byref(p), L.dptr(resp),
                                         L.iptr(counts) if counts is not None else None, None, 0, None, None, None, None), ctx.handle)
            rows = np.arange(n, dtype=np.int64)
            xyz = _positions(cloud, host, rows, ctx)
            intensity = resp
    finally:
        if own is not None:
            own.free()
    out = np.empty((len(rows), 4), dtype=np.float32)
    out[:, :3] = xyz
    out[:, 3] = intensity
    ret = (out,)
    if return_indices:
        ret += (rows,)
    if return_details:
        details.update(response=resp, counts=counts)
        ret += (details,)
    return ret[0] if len(ret) == 1 else ret


def keypointIss(points, iss_salient_radius=3.0, iss_non_max_radius=2.0, iss_gamma_21=0.975, iss_gamma_32=0.975, iss_min_neighbors=5, threads=0, *,
                return_indices=False, return_details=False, ctx=None):
    """keypoints.cpp:112-134 (pcl::ISSKeypoint3D, no border estimation) -> float32 (K,3), in ascending row.  ``threads`` is accepted and
    ignored.  Keyword-only: ``return_indices`` adds the caller rows (K,) int64; ``return_details`` a dict with ``e3`` (N,) float64 -- the
    score: the smallest eigenvalue of the scatter where the eigenvalue rules hold, else 0 -- and ``counts`` (N,) int32, the rows within
    ``iss_non_max_radius``."""
    del threads
    ctx = ctx or default_context()
    cloud, own, host = _cloud(points, ctx)
    try:
        n = cloud.n
        e3 = np.empty(n, dtype=np.float64) if return_details else None
        counts = np.empty(n, dtype=np.int32) if return_details else None
        kp = np.empty(n, dtype=np.int32)
        nk = C.c_int64()
        L.check(L.lib().pcr_iss_pcl(ctx.handle, cloud.handle, float(iss_salient_radius), float(iss_non_max_radius), float(iss_gamma_21), float(iss_gamma_32),
                                    int(iss_min_neighbors), L.dptr(e3) if return_details else None, L.iptr(counts) if return_details else None, L.iptr(kp), n,
                                    C.byref(nk)), ctx.handle)
        rows = kp[: nk.value].astype(np.int64)
        out = _positions(cloud, host, rows, ctx).astype(np.float32)
    finally:
        if own is not None:
            own.free()
    ret = (out,)
    if return_indices:
        ret += (rows,)
    if return_details:
        ret += ({"e3": e3, "counts": counts},)
    return ret[0] if len(ret) == 1 else ret


def keypointHarris6D(points, radius=0.5, nms_threshold=0.001, threads=0, is_nms=False, is_refine=False):
    """keypoints.cpp:162-186.  Not provided."""
    raise NotImplementedError("keypointHarris6D needs colour input (XYZRGB rows and PCL's intensity-gradient covariance); only the XYZ detectors are on the device")


def keypointSift(points, min_scale=0.1, n_octaves=6, n_scales_per_octave=10, min_contrast=0.05):
    """keypoints.cpp:188-211.  Not provided."""
    raise NotImplementedError("keypointSift needs a scale space (PCL's octaves of voxel grids and difference-of-Gaussians over curvature), which is not on the device")


def _no_descriptor(name):
    if name.startswith("featureFPFH33"):
        raise NotImplementedError(f"{name} is not routed yet: the PCL-rule FPFH descriptor is pcl_features.fpfh33 / fpfh33_with_normal (same arguments), "
                                  "compute_fpfh_feature the Open3D-rule one")
    raise NotImplementedError(f"{name} is not routed yet: the PCL-rule SHOT descriptor is pcl_features.shot352 / shot352_with_normal (same arguments)")


def featureFPFH33(pointcloud, keypoints, compute_normal_k=10, feature_radius=1.0):
    _no_descriptor("featureFPFH33")


def featureFPFH33WithNormal(pointcloud, normals, keypoints, feature_radius=1.0):
    _no_descriptor("featureFPFH33WithNormal")


def featureSHOT352(pointcloud, keypoints, compute_normal_k=10, feature_radius=1.0):
    _no_descriptor("featureSHOT352")


def featureSHOT352WithNormal(pointcloud, normals, keypoints, feature_radius=1.0):
    _no_descriptor("featureSHOT352WithNormal")
