"""Object batches for the classifier: ``preprocess`` of Final_Project/scripts/detect.py:269-354 (same name, same config keys, same
return value) with the per-object reductions on the device (include/pcr.h, "object batches").

The labelled rows of a cloud are grouped by object id on the device; counts, means and boxes (``object_stats``) and the resampling
weights ``squareform(pdist(P_o)).mean(axis=0)`` (``resample_weights``, the call of generating-training-set.py:186-189) are computed
there in the reference's operation order, so they carry the reference's bits.  The normalisation ``w /= w.sum()`` and the draw
``np.random.choice`` stay on the host and run in the reference's object order: the global ``np.random`` state ends where the
reference leaves it.  ``preprocess`` gathers the B*S sampled rows in NumPy; ``preprocess_device`` has the pack kernel write the
``(B, S, 6)`` float32 batch straight into a torch tensor on the context's device, ready for ``pointnet2_modules``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .device import DeviceCloud, default_context, points_of

__all__ = ["ObjectBatch", "object_stats", "resample_weights", "preprocess", "preprocess_device", "predict", "TILE"]

TILE = L.PCR_OBJECTS_TILE   # rows j per stage of the weights kernel (include/pcr.h)
_u8p = C.POINTER(C.c_uint8)


def calib_struct(calib):
    """read_calib's dict (extract.py:49-84) -> pcr_kitti_calib; the shapes are checked here, finiteness by the library."""
    cal = L.KittiCalib()
    for key, shape in (("R0_rect", (3, 3)), ("Tr_velo_to_cam", (3, 4)), ("P2", (3, 4))):
        m = np.asarray(calib[key], dtype=np.float64)
        if m.shape != shape:
            raise ValueError(f"calibration entry {key}: expected shape {shape}, got {m.shape}")
        getattr(cal, key)[:] = m.reshape(-1).tolist()
    return cal


class ObjectBatch:
    """The labelled rows of a device cloud grouped by object (pcr_objects): ``offsets`` (n_objects + 1,), ``m`` labelled rows."""

    def __init__(self, cloud, object_ids, n_objects=None, ctx=None):
        ctx = ctx or cloud.ctx
        ids = np.asarray(object_ids)
        if ids.ndim != 1 or ids.shape[0] != cloud.n:
            raise ValueError(f"expected {cloud.n} object ids, one per row, got shape {ids.shape}")
        if ids.dtype.kind not in "iu":
            raise ValueError(f"object ids must be integers, not {ids.dtype}")
        if n_objects is None:
            n_objects = int(ids.max()) + 1 if ids.size else 0
        n_objects = max(int(n_objects), 0)
        if n_objects > 2**31 - 1 or (ids.size and int(ids.max()) >= n_objects):
            raise L.PcrError(L.PCR_E_INVALID)
        labels = np.ascontiguousarray(np.maximum(ids.astype(np.int64), -1), dtype=np.int32)   # (every negative id is noise)
        self.ctx = ctx
        self.n = cloud.n
        self.n_objects = n_objects
        self._h = C.c_void_p()
        L.check(L.lib().pcr_objects_build(ctx.handle, cloud.handle, L.iptr(labels), n_objects, C.byref(self._h)), ctx.handle)
        self.offsets = np.zeros(n_objects + 1, dtype=np.int64)
        L.check(L.lib().pcr_objects_offsets(self.handle, L.lptr(self.offsets)), ctx.handle)
        self.m = int(self.offsets[-1])
        self._grouped_rows = None

    @property
    def handle(self):
        if not self._h:
            raise RuntimeError("object batch freed")
        return self._h

    def rows(self):
        """(m,) int32: the caller rows object by object, ascending within each."""
        rows = np.empty(self.m, dtype=np.int32)
        L.check(L.lib().pcr_objects_rows(self.ctx.handle, self.handle, L.iptr(rows)), self.ctx.handle)
        return rows

    def stats(self):
        k = self.n_objects
        count = np.zeros(k, dtype=np.int64)
        mean, lo, hi = np.zeros((k, 3)), np.zeros((k, 3)), np.zeros((k, 3))
        L.check(L.lib().pcr_objects_stats(self.ctx.handle, self.handle, L.lptr(count), L.dptr(mean), L.dptr(lo), L.dptr(hi)), self.ctx.handle)
        return {"count": count, "mean": mean, "min_bound": lo, "max_bound": hi}

    def weights(self, keep=None):
        """(m,) float64 in the grouped order, unnormalised; 0 for the rows of objects whose `keep` flag is 0."""
        w = np.zeros(self.m, dtype=np.float64)
        kp = None
        if keep is not None:
            keep = np.ascontiguousarray(keep, dtype=np.uint8)
            if keep.shape != (self.n_objects,):
                raise ValueError(f"expected {self.n_objects} keep flags, got shape {keep.shape}")
            kp = keep.ctypes.data_as(_u8p)
        L.check(L.lib().pcr_objects_weights(self.ctx.handle, self.handle, kp, L.dptr(w)), self.ctx.handle)
        return w

    def pack(self, slot_object, local_idx, out_ptr, normals=None):
        """Fill the (b, S, 6 or 3) float32 block at the device address `out_ptr`; returns once it is written."""
        slot = np.ascontiguousarray(slot_object, dtype=np.int32)
        idx = np.ascontiguousarray(local_idx, dtype=np.int64)
        if slot.ndim != 1 or idx.ndim != 2 or idx.shape[0] != slot.shape[0]:
            raise ValueError(f"expected (b,) objects and (b, S) indices, got shapes {slot.shape} and {idx.shape}")
        nrm = None
        if normals is not None:
            nrm = L.as_f64(normals)
            if nrm.shape != (self.n, 3):
                raise ValueError(f"expected ({self.n}, 3) normals, got shape {nrm.shape}")
        L.check(L.lib().pcr_objects_pack_f32(self.ctx.handle, self.handle, L.dptr(nrm) if nrm is not None else None, L.iptr(slot), L.lptr(idx),
                                             idx.shape[0], idx.shape[1], C.c_void_p(out_ptr)), self.ctx.handle)

    def kitti_boxes(self, calib, keep=None):
        """(n_objects, 16) float64, the rows of pcr_objects_kitti_boxes (include/pcr.h, "KITTI boxes"): left, top, right, bottom,
        height, width, length, centre (3), cs, sn, a, b, c, count.  `calib`: read_calib's dict (``R0_rect``, ``Tr_velo_to_cam``,
        ``P2``).  Objects without rows or with a `keep` flag of 0 are NaN up to the count."""
        cal = calib_struct(calib)
        boxes = np.zeros((self.n_objects, L.PCR_KITTI_BOX_DOUBLES), dtype=np.float64)
        kp = None
        if keep is not None:
            keep = np.ascontiguousarray(keep, dtype=np.uint8)
            if keep.shape != (self.n_objects,):
                raise ValueError(f"expected {self.n_objects} keep flags, got shape {keep.shape}")
            kp = keep.ctypes.data_as(_u8p)
        L.check(L.lib().pcr_objects_kitti_boxes(self.ctx.handle, self.handle, C.byref(cal), kp, L.dptr(boxes)), self.ctx.handle)
        return boxes

    def match_labels(self, calib, labels):
        """pcr_objects_match_labels (include/pcr.h, "label match") for `labels`, an (L,16) array of label records -> dict with one
        entry per label: ``k`` rows of any object in the label's sphere, ``object_id`` the object with the most rows in the label's
        box (the lowest id on a tie, -1: none), ``votes`` its rows in the box, ``count`` its rows in the sphere (the selected rows),
        ``center`` (L,3) their centre (NaN without an object), ``positions`` a list of int64 arrays, the places of the selected rows
        within the object in ascending caller row, unpacked from the ballot words, ``rows`` their caller rows."""
        rec = np.ascontiguousarray(labels, dtype=np.float64)
        if rec.ndim != 2 or rec.shape[1] != L.PCR_LABEL_DOUBLES:
            raise ValueError(f"expected (L, {L.PCR_LABEL_DOUBLES}) label records, got shape {rec.shape}")
        n = rec.shape[0]
        cal = calib_struct(calib)
        counts = np.diff(self.offsets)
        words = max(int(-(-int(counts.max()) // 64)) if len(counts) else 0, 1)
        result = np.zeros((n, L.PCR_LABEL_RESULT_DOUBLES), dtype=np.float64)
        bits = np.zeros((n, words), dtype=np.uint64)
        L.check(L.lib().pcr_objects_match_labels(self.ctx.handle, self.handle, C.byref(cal), L.dptr(rec), n, L.dptr(result),
                                                 bits.ctypes.data_as(C.POINTER(C.c_uint64)), words), self.ctx.handle)
        object_id = result[:, 1].astype(np.int64)
        unpacked = np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")   # (the words are little-endian on every host of a gfx950)
        positions = [np.flatnonzero(row).astype(np.int64) for row in unpacked]
        if self._grouped_rows is None and (object_id >= 0).any():
            self._grouped_rows = self.rows().astype(np.int64)   # (the handle never changes: one read-back serves every later call)
        grouped = self._grouped_rows
        rows = [grouped[self.offsets[o] + p] if o >= 0 else np.zeros(0, dtype=np.int64) for o, p in zip(object_id, positions)]
        return {"k": result[:, 0].astype(np.int64), "object_id": object_id, "votes": result[:, 2].astype(np.int64), "count": result[:, 3].astype(np.int64),
                "center": result[:, 4:7].copy(), "positions": positions, "rows": rows}

    def free(self):
        if self._h:
            L.lib().pcr_objects_free(self.ctx.handle, self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.free()
        except Exception:
            pass


def select(count, mean, max_radius_distance, min_count=4):
    """detect.py:286-292 through pcr_objects_select -> bool (n_objects,): more than `min_count` rows and the centre within the radius."""
    count = np.ascontiguousarray(count, dtype=np.int64)
    mean = L.as_f64(mean)
    if count.ndim != 1 or mean.shape != (count.shape[0], 3):
        raise ValueError(f"expected (k,) counts and (k, 3) means, got shapes {count.shape} and {mean.shape}")
    keep = np.zeros(count.shape[0], dtype=np.uint8)
    L.check(L.lib().pcr_objects_select(L.lptr(count), L.dptr(mean), count.shape[0], int(min_count), float(max_radius_distance), keep.ctypes.data_as(_u8p)))
    return keep.astype(bool)


def _ids(object_ids):
    ids = np.asarray(object_ids)
    if ids.size == 0:
        raise ValueError("object_ids is empty: max() of an empty sequence")   # detect.py:279
    return ids.reshape(-1) if ids.ndim != 1 else ids


def _as_cloud(data, ctx):
    """-> (DeviceCloud, owned)."""
    if isinstance(data, DeviceCloud):
        return data, False
    arr = points_of(data)
    if arr.shape[0] == 0:
        raise L.PcrError(L.PCR_E_EMPTY)
    return DeviceCloud.upload(np.ascontiguousarray(arr[:, :3]), ctx or default_context()), True


def object_stats(data, object_ids, ctx=None):
    """Per object id 0 .. max(object_ids): ``count`` (k,) int64, ``mean`` (k,3) = np.mean(points[object_ids == o], axis=0) bit for bit,
    ``min_bound`` / ``max_bound`` (k,3), the box detect.py:244 draws.  An id without rows: count 0, mean NaN, bounds +inf / -inf."""
    ids = _ids(object_ids)
    cloud, owned = _as_cloud(data, ctx)
    batch = None
    try:
        batch = ObjectBatch(cloud, ids, ctx=ctx)
        return batch.stats()
    finally:
        if batch is not None:
            batch.free()
        if owned:
            cloud.free()


def resample_weights(data, object_ids=None, ctx=None):
    """(n,) float64 by caller row: ``squareform(pdist(P_o, 'euclidean')).mean(axis=0)`` of the row's object, unnormalised, bit for
    bit, without the n x n matrix; 0 for noise rows.  ``object_ids=None``: the whole cloud is one object
    (generating-training-set.py:186-189)."""
    ids = None if object_ids is None else _ids(object_ids)
    cloud, owned = _as_cloud(data, ctx)
    batch = None
    try:
        batch = ObjectBatch(cloud, np.zeros(cloud.n, dtype=np.int32) if ids is None else ids, ctx=ctx)
        out = np.zeros(cloud.n, dtype=np.float64)
        out[batch.rows()] = batch.weights()
        return out
    finally:
        if batch is not None:
            batch.free()
        if owned:
            cloud.free()


def _inputs(segmented_objects, normals):
    """-> (points: DeviceCloud or (n,3) array, normals (n,3) float64 or None)."""
    if isinstance(segmented_objects, DeviceCloud):
        pts = segmented_objects
    elif isinstance(segmented_objects, (tuple, list)) and len(segmented_objects) == 2:
        pts, nrm = segmented_objects
        normals = nrm if normals is None else normals
        if not isinstance(pts, DeviceCloud):
            pts = points_of(pts)
    else:
        if normals is None:
            normals = getattr(segmented_objects, "normals", None)
        pts = points_of(segmented_objects)
    n = pts.n if isinstance(pts, DeviceCloud) else pts.shape[0]
    if normals is not None:
        normals = L.as_f64(np.asarray(normals))
        if normals.shape != (n, 3):
            raise ValueError(f"expected ({n}, 3) normals, got shape {normals.shape}")
    return pts, normals


def _sample(segmented_objects, object_ids, config, ctx, normals):
    """Everything up to the draw: -> (batch, cloud, owned, host points or None, normals, kept ids, [idx per kept object], stats)."""
    ids = _ids(object_ids)
    S = int(config["num_sample_points"])
    batch_size = int(config["batch_size"])
    max_radius = float(config["max_radius_distance"])
    if S < 1 or batch_size < 1:
        raise ValueError("num_sample_points and batch_size must be positive")
    pts, normals = _inputs(segmented_objects, normals)
    host_points = None if isinstance(pts, DeviceCloud) else pts
    n = len(pts)
    if ids.shape[0] != n:
        raise ValueError(f"expected {n} object ids, one per row, got {ids.shape[0]}")
    if ids.dtype.kind not in "iu":
        raise ValueError(f"object ids must be integers, not {ids.dtype}")
    cloud, owned = _as_cloud(pts, ctx)
    batch = None
    try:
        batch = ObjectBatch(cloud, ids, ctx=ctx)
        st = batch.stats()
        keep = select(st["count"], st["mean"], max_radius)
        w_all = batch.weights(keep) if keep.any() else None
        kept, draws = [], []
        for o in np.flatnonzero(keep):   # ascending ids: the reference's loop order
            a, b = int(batch.offsets[o]), int(batch.offsets[o + 1])
            n = b - a
            weights = w_all[a:b].copy()
            weights /= weights.sum()                                                          # detect.py:302
            draws.append(np.random.choice(np.arange(n), size=(S,), replace=True if S > n else False, p=weights))   # detect.py:304-308
            kept.append(int(o))
        return batch, cloud, owned, host_points, normals, kept, draws, st
    except BaseException:
        if batch is not None:
            batch.free()
        if owned:
            cloud.free()
        raise


def _padded(kept, batch_size):
    """detect.py:327-333: copies of the first kept object up to a multiple of the batch size."""
    N = len(kept)
    slots = list(range(N))
    if N % batch_size != 0:
        slots += [0] * (batch_size - N % batch_size)
    return slots, N


def preprocess(segmented_objects, object_ids, config, ctx=None, *, normals=None):
    """detect.py:269-354 -> ``(dataset, N)``: ``dataset`` a list of ``(X, object_id)`` with X (num_sample_points, 6) float64 =
    ``hstack(points_[idx] - points_.mean(axis=0), normals_[idx])``, padded with copies of the first kept object to a multiple of
    ``config['batch_size']``; N the unpadded count.  Objects with at most 4 points or a centre beyond
    ``config['max_radius_distance']`` are skipped.

    `segmented_objects`: an object with ``.points`` and ``.normals`` (Open3D style), a ``(points, normals)`` pair, or a DeviceCloud
    with ``normals=``; without normals X has 3 columns.  Counts, means and resampling weights come from the device with the
    reference's bits; ``np.random.choice`` is called once per kept object in ascending id order, like the reference.  Empty
    `object_ids`: ValueError; nothing kept: ``([], 0)``; an object whose points all coincide has weights 0/0 and
    ``np.random.choice`` raises its ValueError, as in the reference."""
    batch, cloud, owned, host_points, normals, kept, draws, st = _sample(segmented_objects, object_ids, config, ctx, normals)
    try:
        if not kept:
            return [], 0
        rows = batch.rows()
        points = cloud.download() if host_points is None else np.asarray(host_points[:, :3], dtype=np.float64)
        X = []
        for o, idx in zip(kept, draws):
            r = rows[batch.offsets[o]:batch.offsets[o + 1]][idx]
            cols = [points[r] - st["mean"][o]]
            if normals is not None:
                cols.append(normals[r])
            X.append(np.hstack(cols))
        slots, N = _padded(kept, int(config["batch_size"]))
        return [(X[s], kept[s]) for s in slots], N
    finally:
        batch.free()
        if owned:
            cloud.free()


def preprocess_device(segmented_objects, object_ids, config, ctx=None, *, normals=None):
    """``preprocess`` with the batch written on the device -> ``(X, object_ids, N)``: X a ``(B_padded, num_sample_points, 6)`` float32
    torch tensor on the context's device (3 channels without normals), bit-equal to ``torch.from_numpy(np.stack(X_ref)).float()``;
    ``object_ids`` (B_padded,) int64, the id behind every slot; N the unpadded count.  Nothing kept: an empty tensor and N = 0."""
    import torch   # lazily: importing the package does not import torch

    batch, cloud, owned, host_points, normals, kept, draws, st = _sample(segmented_objects, object_ids, config, ctx, normals)
    try:
        S = int(config["num_sample_points"])
        channels = 6 if normals is not None else 3
        device = torch.device("cuda", batch.ctx.device)
        slots, N = _padded(kept, int(config["batch_size"]))
        X = torch.empty((len(slots), S, channels), dtype=torch.float32, device=device)
        if slots:
            torch.cuda.current_stream(device).synchronize()   # the tensor's memory may still be in use by work queued earlier
            batch.pack([kept[s] for s in slots], np.stack([draws[s] for s in slots]), X.data_ptr(), normals)
        return X, np.array([kept[s] for s in slots], dtype=np.int64), N
    finally:
        batch.free()
        if owned:
            cloud.free()


def predict(X, object_ids, N, model, config):
    """detect.py:357-412 behind its ``preprocess`` -> ``{class_id: {object_id: confidence}}`` for ``class_id`` in
    ``range(config['num_classes'])``.  ``X, object_ids, N`` are what ``preprocess_device`` returns: the (B_padded, S, channels) float32
    batch, the id behind every slot and the unpadded count.  The model (put into eval mode, as the reference does) sees whole batches
    of ``config['batch_size']`` slots under ``torch.no_grad()`` -- a classifier of ``pointnet2_models`` then runs its fused path --
    and every slot gets ``argmax`` and ``max`` of the softmax of its logits.  Slots from N on are padding and are skipped; the
    entries are inserted in slot order, the reference's.  N = 0: every class has an empty dict and the model is not called."""
    import torch   # lazily: importing the package does not import torch
    import torch.nn.functional as F

    predictions = {class_id: {} for class_id in range(int(config["num_classes"]))}
    batch_size = int(config["batch_size"])
    N = int(N)
    if N <= 0:
        return predictions
    if N > len(X) or len(object_ids) != len(X):
        raise ValueError(f"X has {len(X)} slots and object_ids {len(object_ids)}, N is {N}")
    if hasattr(model, "eval"):
        model.eval()
    for first in range(0, (len(X) // batch_size) * batch_size, batch_size):
        if first >= N:
            break
        with torch.no_grad():
            logits = model(X[first:first + batch_size])
        prob_score = F.softmax(logits, dim=1).cpu().numpy()
        for slot, class_id, confidence in zip(range(first, min(first + batch_size, N)), np.argmax(prob_score, axis=1), np.max(prob_score, axis=1)):
            predictions[int(class_id)][object_ids[slot]] = confidence
    return predictions
