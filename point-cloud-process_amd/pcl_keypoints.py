"""SIFT-3D, the scale-aware detector of the reference's pybind module PCLKeypoint (``keypointSift``, PCLKeypoints/src/keypoints.cpp:85-109:
pcl::SIFTKeypoint on the y coordinate) on the device, under names of its own: ``sift_keypoints`` (the octave loop) and the stages under
it, ``sift_octave``, ``sift_extrema`` and ``sift_scales``.  The rules are stated in include/pcr.h (pcr_sift, pcr_sift_octave,
pcr_sift_extrema, pcr_sift_scales) and restated in NumPy by tests/sift_checks.py.  PCL itself is not used and no version of it is pinned:
parity with its binary32 output is unpinned.  One stated departure: an octave is down-sampled by this project's voxel filter (Open3D's
rule, ``voxel_down_sample``), not by PCL's VoxelGrid lattice.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .device import DeviceCloud, default_context, points_of

__all__ = ["sift_keypoints", "sift_octave", "sift_extrema", "sift_scales"]

_FIELDS = {"x": 0, "y": 1, "z": 2, 0: 0, 1: 1, 2: 2}


def _checked(points):
    """A DeviceCloud as it is, anything else as (N,3) float64; rows with a coordinate that is not finite are refused (before a device is
    asked for, when the points are on the host).  A DeviceCloud is DOWNLOADED for the test, 24 bytes a row and a wait in every call (the
    library keeps no finiteness flag of a resident cloud).  That cost is inside every time profiles/sift_bench.json gives for the Python
    calls, and the file gives it on its own (``finite_check_download_wall_ms``)."""
    if isinstance(points, DeviceCloud):
        host = points.download()
    else:
        points = host = np.ascontiguousarray(points_of(points)[:, :3], dtype=np.float64)
    if not np.isfinite(host).all():
        raise ValueError("the cloud holds a coordinate that is not finite")
    return points


def _cloud(points, ctx):
    """-> (DeviceCloud, the one to free or None) of what _checked returned."""
    if isinstance(points, DeviceCloud):
        return points, None
    c = DeviceCloud.upload(points, ctx)
    return c, c


def _field(field):
    try:
        return _FIELDS[field]
    except (KeyError, TypeError):
        raise ValueError(f"field must be 'x', 'y' or 'z' (0, 1, 2), got {field!r}") from None


def _with_capacity(call, first):
    """call(capacity) -> (status, needed); a buffer that was too small is the only PCR_E_UNSUPPORTED that is answered, by one more call."""
    capacity = max(int(first), 1)
    status, needed = call(capacity)
    if status == L.PCR_E_UNSUPPORTED and needed > capacity:
        status, needed = call(needed)
    return status, needed


def sift_scales(base_scale, n_scales_per_octave):
    """The scales of one octave -> (q + 3,) float64: base_scale * 2 ** ((s - 1) / q)."""
    q = int(n_scales_per_octave)
    out = np.empty(max(q, 0) + 3, dtype=np.float64)
    L.check(L.lib().pcr_sift_scales(float(base_scale), q, L.dptr(out)), None, soft=())
    return out


def sift_octave(points, base_scale, n_scales_per_octave=10, min_contrast=0.05, *, field="y", return_dog=True, ctx=None):
    """One octave on the cloud as given (no down-sampling) -> (rows (K,) int64, columns (K,) int64, info): the entries (row, c) that are
    scale-space extrema, in ascending (row, c); the keypoint's scale is ``sift_scales(...)[c]``.  ``info``: {"dog": (N, q + 2) float64
    differences of adjacent scales, "counts": (N,) int32 rows in every ball} (``return_dog=False``: an empty dict)."""
    f = _field(field)
    points = _checked(points)
    ctx = ctx or default_context()
    cloud, own = _cloud(points, ctx)
    try:
        n, q = cloud.n, int(n_scales_per_octave)
        dog = np.empty((n, max(q, 0) + 2), dtype=np.float64) if return_dog else None
        counts = np.empty(n, dtype=np.int32) if return_dog else None
        out = {}

        def call(capacity):
            rows, cols, nk = np.empty(capacity, dtype=np.int32), np.empty(capacity, dtype=np.int32), C.c_int64(0)
            st = L.lib().pcr_sift_octave(ctx.handle, cloud.handle, float(base_scale), q, float(min_contrast), f, L.dptr(dog) if return_dog else None,
                                         L.iptr(counts) if return_dog else None, L.iptr(rows), L.iptr(cols), capacity, C.byref(nk))
            out["rows"], out["cols"] = rows, cols
            return st, int(nk.value)

        st, k = _with_capacity(call, n)
        L.check(st, ctx.handle, soft=())
    finally:
        if own is not None:
            own.free()
    info = {"dog": dog, "counts": counts} if return_dog else {}
    return out["rows"][:k].astype(np.int64), out["cols"][:k].astype(np.int64), info


def sift_extrema(points, dog, min_contrast=0.05, *, ctx=None):
    """The extrema stage alone on a table ``dog`` (N, C) of the caller's, 3 <= C <= 15 -> (rows (K,) int64, columns (K,) int64)."""
    points = _checked(points)
    ctx = ctx or default_context()
    cloud, own = _cloud(points, ctx)
    try:
        n = cloud.n
        table = L.as_f64(np.asarray(dog, dtype=np.float64))
        if table.ndim != 2 or table.shape[0] != n:
            raise ValueError("the table does not match the cloud")
        out = {}

        def call(capacity):
            rows, cols, nk = np.empty(capacity, dtype=np.int32), np.empty(capacity, dtype=np.int32), C.c_int64(0)
            st = L.lib().pcr_sift_extrema(ctx.handle, cloud.handle, L.dptr(table), int(table.shape[1]), float(min_contrast), L.iptr(rows), L.iptr(cols), capacity,
                                          C.byref(nk))
            out["rows"], out["cols"] = rows, cols
            return st, int(nk.value)

        st, k = _with_capacity(call, n)
        L.check(st, ctx.handle, soft=())
    finally:
        if own is not None:
            own.free()
    return out["rows"][:k].astype(np.int64), out["cols"][:k].astype(np.int64)


def sift_keypoints(points, min_scale=0.1, n_octaves=6, n_scales_per_octave=10, min_contrast=0.05, *, field="y", return_scales=False, return_details=False,
                   ctx=None):
    """keypointSift (keypoints.cpp:85-109) with the wrapper's defaults -> float32 (K,3): the scale-space extrema of the ``field``
    coordinate over ``n_octaves`` octaves, each the voxel down-sampling (leaf = its base scale, which doubles) of the one before;
    keypoints in ascending (octave, row, column), their positions the octave's down-sampled rows.  ``points``: (N,>=3) array-like, an
    object with ``.points``, or a DeviceCloud; a coordinate that is not finite is a ValueError.

    Keyword-only: ``return_scales`` adds (K,) float64 scales; ``return_details`` adds a dict with ``octave`` (K,), ``row`` (K,) of that
    octave's cloud, ``column`` (K,) and ``octave_sizes`` (n_octaves,) rows of every octave's cloud, 0 for the octaves not run."""
    f = _field(field)
    points = _checked(points)
    ctx = ctx or default_context()
    cloud, own = _cloud(points, ctx)
    try:
        n, q, n_oct = cloud.n, int(n_scales_per_octave), int(n_octaves)
        sizes = np.zeros(max(n_oct, 1), dtype=np.int64)
        out = {}

        def call(capacity):
            kp, octave, row, nk = np.empty((capacity, 4), dtype=np.float64), np.empty(capacity, dtype=np.int32), np.empty(capacity, dtype=np.int32), C.c_int64(0)
            st = L.lib().pcr_sift(ctx.handle, cloud.handle, float(min_scale), n_oct, q, float(min_contrast), f, L.dptr(kp), L.iptr(octave), L.iptr(row), capacity,
                                  C.byref(nk), L.lptr(sizes))
            out["kp"], out["octave"], out["row"] = kp, octave, row
            return st, int(nk.value)

        st, k = _with_capacity(call, n)
        L.check(st, ctx.handle, soft=())
    finally:
        if own is not None:
            own.free()
    kp = out["kp"][:k]
    res = [kp[:, :3].astype(np.float32)]
    if return_scales:
        res.append(kp[:, 3].copy())
    if return_details:
        octave = out["octave"][:k].astype(np.int64)
        column = np.empty(k, dtype=np.int64)
        for o in np.unique(octave):
            # a keypoint's scale is entry `column` of pcr_sift_scales(min_scale * 2^o, q), the very table the library took it from (doubling
            # is exact): the column is where it is found, to the bit
            sel = octave == o
            hit = kp[sel, 3][:, None] == sift_scales(float(min_scale) * 2.0 ** int(o), q)[None, :]
            if not (hit.sum(axis=1) == 1).all():
                raise RuntimeError("a keypoint's scale is not one of its octave's scales")
            column[sel] = np.argmax(hit, axis=1)
        res.append({"octave": octave, "row": out["row"][:k].astype(np.int64), "column": column, "octave_sizes": sizes[:n_oct].copy()})
    return res[0] if len(res) == 1 else tuple(res)
