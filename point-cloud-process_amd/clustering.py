"""Ground removal + clustering of a lidar sweep: Cluster_dbscan/clustering.py (same function names, same defaults).

``ground_segmentation`` is the RANSAC plane fit of clustering.py:36-95 on the device (include/pcr.h: pcr_ground_segmentation),
``clustering`` the DBSCAN of clustering.py:98-132 and ``segment_and_cluster`` the body of its main() loop (clustering.py:158-160)
with the intermediate cloud kept on the device.  The sweep reader of clustering.py:22-33 is ``read_velodyne_bin`` in registration.py.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .dbscan import DBSCAN
from .device import DeviceCloud, default_context, points_of

__all__ = ["ground_segmentation", "clustering", "segment_and_cluster", "tau", "N", "ratio"]

# clustering.py:17-19
tau = 0.6
N = 35
ratio = 0.5


def _segment(cloud, samples, tau_, ratio_, *, want_cloud, want_rows, want_mask):
    """pcr_ground_segmentation on a DeviceCloud -> (outlier DeviceCloud or None, info dict)."""
    smp = np.ascontiguousarray(samples, dtype=np.int64)
    if smp.ndim != 2 or smp.shape[1] != 3:
        raise ValueError(f"expected (N, 3) sample rows, got shape {smp.shape}")
    ctx = cloud.ctx
    n = cloud.n
    n_hyp = smp.shape[0]
    p = L.GroundParams()
    L.lib().pcr_ground_default_params(C.byref(p))
    p.tau = float(tau_)
    p.ratio = float(ratio_)
    p.n_hyp = int(n_hyp)
    res = L.GroundResult()
    counts = np.zeros(max(n_hyp, 1), dtype=np.int64)
    rows = np.empty(n, dtype=np.int32) if want_rows else None
    mask = np.empty(n, dtype=np.uint8) if want_mask else None
    h = C.c_void_p()
    st = L.lib().pcr_ground_segmentation(
        ctx.handle, cloud.handle, L.lptr(smp), C.byref(p), C.byref(h) if want_cloud else None, L.iptr(rows) if want_rows else None,
        mask.ctypes.data_as(C.POINTER(C.c_uint8)) if want_mask else None, L.lptr(counts), C.byref(res))
    info = {"best_hyp": int(res.best_hyp), "evaluated": int(res.evaluated), "counts": counts[:n_hyp]}
    if st == L.PCR_E_TOO_FEW_ASSOC:
        # clustering.py:83 indexes with best_outliers = None when no trial ever had an inlier
        err = ValueError("ground_segmentation: every sampled triple is degenerate (repeated or collinear points), no plane to remove")
        err.info = info
        raise err
    L.check(st, ctx.handle, soft=())
    m = int(res.n_outliers)
    info.update(n_inliers=int(res.n_inliers), n_outliers=m, point=np.array(res.point[:]), normal=np.array(res.normal[:]))
    if want_rows:
        info["outlier_rows"] = rows[:m].copy()
    if want_mask:
        info["inlier_mask"] = mask.astype(bool)
    return (DeviceCloud(ctx, h, m) if want_cloud else None), info


def _draw(n, n_trials):
    """clustering.py:57, one call per trial: the reference's stream of draws."""
    return np.array([np.random.randint(0, n, size=3) for _ in range(n_trials)], dtype=np.int64).reshape(n_trials, 3)


def _run(cloud, samples, tau_, n_hyp, ratio_, **want):
    """With samples=None: draw like the reference and leave np.random where ITS loop would (it stops drawing at the break)."""
    if samples is not None:
        return _segment(cloud, samples, tau_, ratio_, **want)
    n_hyp = int(n_hyp)
    if n_hyp < 1:
        raise L.PcrError(L.PCR_E_INVALID)
    state = np.random.get_state()
    out = _segment(cloud, _draw(cloud.n, n_hyp), tau_, ratio_, **want)   # (every trial degenerate: the reference drew all N, so do we)
    np.random.set_state(state)
    _draw(cloud.n, out[1]["evaluated"])
    return out


def _as_cloud(data, ctx):
    """-> (DeviceCloud, host array or None, owned)."""
    if isinstance(data, DeviceCloud):
        return data, None, False
    arr = points_of(data)
    if arr.shape[0] == 0:
        raise L.PcrError(L.PCR_E_EMPTY)
    return DeviceCloud.upload(arr, ctx or default_context()), arr, True


def ground_segmentation(data, tau=tau, N=N, ratio=ratio, *, samples=None, return_info=False, ctx=None):
    """clustering.py:36-95: remove the inliers of the best of N random 3-point planes (|distance| < tau; early break once the
    best plane holds more than `ratio` of the points).  `data`: (n,3) array, object with ``.points`` or DeviceCloud.  An array
    comes back as an array of the input's dtype holding the outlier rows in ascending order (``data[best_outliers]``), a
    DeviceCloud as a new DeviceCloud that never left the device.

    `samples` (N,3) rows: the triples to try, instead of ``np.random.randint(0, n, size=3)`` per trial; without it the global
    np.random state ends exactly where the reference's loop leaves it.  Distances are evaluated in binary64 on the stored
    coordinates (the reference: float32; labels can differ only within rounding of tau).  Every triple
    degenerate -> ValueError.  `return_info`: also a dict with best_hyp, evaluated, counts (all N trials), inlier_mask,
    outlier_rows, point, normal."""
    cloud, arr, owned = _as_cloud(data, ctx)
    try:
        out, info = _run(cloud, samples, tau, N, ratio, want_cloud=arr is None, want_rows=arr is not None or return_info, want_mask=return_info)
    finally:
        if owned:
            cloud.free()
    if arr is not None:
        out = arr[info["outlier_rows"]]
    return (out, info) if return_info else out


def clustering(data, radius=0.5, min_pts=10):
    """clustering.py:98-132, its option 2 (clustering.py:127-130): ``DBSCAN(radius, min_pts)`` of dbscan.py, labels int32 with
    -1 = noise.  Option 1, Open3D's ``cluster_dbscan``, is absent here and has different semantics (border points, numbering)."""
    clus = DBSCAN(radius, min_pts)
    clus.fit(data)
    return clus.predict()


def segment_and_cluster(data, tau=tau, N=N, ratio=ratio, radius=0.5, min_pts=10, *, samples=None, ctx=None):
    """The body of main()'s loop, clustering.py:158-160: ground removal, then clustering of what is left; the segmented cloud goes
    from one step to the next on the device.  -> (segmented_points, labels); segmented_points like ground_segmentation's result."""
    cloud, arr, owned = _as_cloud(data, ctx)
    seg = None
    try:
        seg, info = _run(cloud, samples, tau, N, ratio, want_cloud=True, want_rows=arr is not None, want_mask=False)
        if seg.n > 0:
            clus = DBSCAN(radius, min_pts, ctx=seg.ctx)
            clus.fit(seg)
            labels = clus.predict()
        else:
            labels = np.empty(0, dtype=np.int32)
    finally:
        if owned:
            cloud.free()
        if seg is not None and arr is not None:
            seg.free()
    return (arr[info["outlier_rows"]] if arr is not None else seg), labels
