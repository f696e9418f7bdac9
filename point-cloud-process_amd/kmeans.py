"""K-Means clustering: class K_Means of Cluster_KMeans_GMM/compare_cluster.py:16,105,164-170 (``K_Means(n_clusters=...)``, ``fit``,
``predict``) with Lloyd's iteration on the device (include/pcr.h: pcr_kmeans_fit / pcr_kmeans_predict).

The reference's own KMeans.py is not in its tree; the semantics are the ones include/pcr.h states: direct-form squared distances in
binary64, the lowest cluster on ties, an empty cluster keeps its centre, the loop stops when no centre moved by more than
``tolerance``.  The fitted centres seed ``GMM.fit(means_init=...)``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .gmm import _as_cloud, _as_points

__all__ = ["K_Means"]


class K_Means(object):
    """After ``fit``: ``centers_`` (k,dim), ``labels_`` (n,) by caller row, ``counts_`` (k,), ``inertia_``, ``n_iter_``,
    ``converged_``, ``n_empty_`` (clusters without points), ``inertia_history_`` / ``shift_history_`` (one entry per iteration), ``device_ms_``."""

    def __init__(self, n_clusters=2, tolerance=0.0001, max_iter=300):
        self.n_clusters = n_clusters
        self.tolerance = tolerance
        self.max_iter = max_iter

        self.centers_ = None  # (k, dim)
        self.labels_ = None
        self.counts_ = None
        self.inertia_ = None
        self.n_iter_ = 0
        self.converged_ = False
        self.n_empty_ = 0
        self.inertia_history_ = None
        self.shift_history_ = None
        self.device_ms_ = 0.0
        self._dim = None

    def fit(self, data, *, centers_init=None, dim=None, labels=True, ctx=None):
        """`data`: (n,2) or (n,3) array, object with ``.points``, or a DeviceCloud (dim 3 unless `dim` says 2; nothing is
        downloaded but the k seed rows).  Without `centers_init` (k,dim) exactly one ``np.random.choice(n, k, replace=False)`` is
        drawn on the global stream and those rows are the initial centres (k > n: ``ValueError``, nothing drawn); with it nothing
        is drawn and k may exceed n (the surplus clusters stay empty where they are).  ``labels=False`` skips the label download
        (``labels_`` is None).  n_clusters outside 1..32, a dim other than 2 or 3, max_iter < 1: ``PcrError`` (PCR_E_INVALID).  All
        of these are raised before anything is uploaded."""
        k, max_iter = int(self.n_clusters), int(self.max_iter)
        data, dim = _as_points(data, dim)
        if not (1 <= k <= L.PCR_KMEANS_MAX_K) or dim not in (2, 3) or max_iter < 1:
            raise L.PcrError(L.PCR_E_INVALID, f"n_clusters {k} (1..{L.PCR_KMEANS_MAX_K}), dim {dim} (2 or 3), max_iter {max_iter} (>= 1)")
        if centers_init is not None:
            centers_init = L.as_f64(centers_init)
            if centers_init.shape != (k, dim):
                raise ValueError(f"centers_init: expected shape {(k, dim)}, got {centers_init.shape}")
        elif k > len(data):
            raise ValueError(f"cannot draw {k} distinct seed rows from {len(data)} points: give centers_init")
        cloud, dim, owned = _as_cloud(data, dim, ctx)
        try:
            p = L.KmeansParams()
            L.lib().pcr_kmeans_default_params(C.byref(p))
            p.n_clusters, p.dim, p.max_iter, p.tol = k, dim, max_iter, float(self.tolerance)
            if centers_init is None:
                rows = np.random.choice(cloud.n, k, replace=False)
                centers0 = np.ascontiguousarray(cloud.download_rows(rows)[:, :dim])
            else:
                centers0 = centers_init
            centers, counts = np.empty((k, dim)), np.empty(k, dtype=np.int64)
            lab = np.empty(cloud.n, dtype=np.int32) if labels else None
            inertia_hist, shift_hist = np.empty(p.max_iter), np.empty(p.max_iter)
            res = L.KmeansResult()
            st = L.lib().pcr_kmeans_fit(cloud.ctx.handle, cloud.handle, C.byref(p), L.dptr(centers0), L.dptr(centers), L.lptr(counts),
                                        L.iptr(lab) if labels else None, L.dptr(inertia_hist), L.dptr(shift_hist), C.byref(res))
            L.check(st, cloud.ctx.handle, soft=())
        finally:
            if owned:
                cloud.free()
        self.centers_ = centers
        self.labels_ = lab.astype(np.intp) if labels else None
        self.counts_ = counts
        self.inertia_ = float(res.inertia)
        self.n_iter_ = int(res.iters)
        self.converged_ = bool(res.converged)
        self.n_empty_ = int(res.n_empty)
        self.inertia_history_ = inertia_hist[:res.iters].copy()
        self.shift_history_ = shift_hist[:res.iters].copy()
        self.device_ms_ = float(res.device_ms)
        self._dim = dim
        return self

    def predict(self, data, *, ctx=None):
        """The nearest fitted centre per row (the lowest on ties), like ``np.argmin`` over the squared distances."""
        if self.centers_ is None:
            raise RuntimeError("K_Means.predict before fit")
        cloud, dim, owned = _as_cloud(data, self._dim, ctx)
        try:
            lab = np.empty(cloud.n, dtype=np.int32)
            st = L.lib().pcr_kmeans_predict(cloud.ctx.handle, cloud.handle, int(self.n_clusters), dim, L.dptr(L.as_f64(self.centers_)), L.iptr(lab),
                                            None, None)
            L.check(st, cloud.ctx.handle, soft=())
        finally:
            if owned:
                cloud.free()
        return lab.astype(np.intp)

    def fit_predict(self, data, *, centers_init=None, dim=None, ctx=None):
        return self.fit(data, centers_init=centers_init, dim=dim, ctx=ctx).labels_
