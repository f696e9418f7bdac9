"""Gaussian-mixture clustering: class GMM of Cluster_KMeans_GMM/GMM.py:13-71 (same constructor, ``fit`` / ``predict``, same attribute
shapes) with the EM loop on the device (include/pcr.h: pcr_gmm_fit / pcr_gmm_predict).

Two stated deviations: the densities are evaluated in the log domain, so data far from the initial means -- any lidar
sweep -- does not underflow to 0/0 as it does in the reference; and a component that loses all its points or whose covariance stops
being positive definite raises ``np.linalg.LinAlgError`` where scipy raises inside the reference's loop.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .device import DeviceCloud, default_context

__all__ = ["GMM"]


def _as_points(data, dim):
    """-> (DeviceCloud or (n,3) array, dim), nothing uploaded.  Arrays: (n,2) or (n,3); 2-D rows become (x, y, 0)."""
    if isinstance(data, DeviceCloud):
        return data, 3 if dim is None else int(dim)
    arr = np.asarray(getattr(data, "points", data))
    if arr.ndim != 2:
        raise ValueError(f"expected an (n,2) or (n,3) point array, got shape {arr.shape}")
    if arr.shape[1] not in (2, 3):
        raise L.PcrError(L.PCR_E_INVALID, f"dim {arr.shape[1]}: only 2 and 3 are supported")
    if arr.shape[0] == 0:
        raise L.PcrError(L.PCR_E_EMPTY)
    dim = arr.shape[1] if dim is None else int(dim)
    if dim > arr.shape[1]:
        raise L.PcrError(L.PCR_E_INVALID, f"dim {dim} asked of {arr.shape[1]}-column data")
    if arr.shape[1] == 2:
        if arr.dtype != np.float32:
            arr = arr.astype(np.float64)
        arr = np.column_stack([arr, np.zeros(len(arr), dtype=arr.dtype)])
    return arr, dim


def _as_cloud(data, dim, ctx):
    """-> (DeviceCloud, dim, owned): a DeviceCloud as it is, anything else uploaded."""
    pts, dim = _as_points(data, dim)
    if isinstance(pts, DeviceCloud):
        return pts, dim, False
    return DeviceCloud.upload(pts, ctx or default_context()), dim, True


class GMM(object):
    """GMM.py:13-21.  After ``fit``: ``means`` (k,dim), ``covs`` (k,dim,dim), ``weights`` (k,1) like the reference, and ``n_iter_``,
    ``nll_`` (negative log-likelihood of the fitted parameters), ``nll_history_`` (after every iteration), ``converged_``."""

    def __init__(self, n_clusters, max_iter=50, tol=0.001):
        self.n_clusters = n_clusters
        self.max_iter = max_iter

        self.means = None  # (k, dim)
        self.covs = None  # (k, dim, dim)
        self.weights = np.ones((n_clusters, 1)) / n_clusters
        self.tol = tol
        self.n_iter_ = 0
        self.nll_ = None
        self.nll_history_ = None
        self.converged_ = False
        self.device_ms_ = 0.0
        self._dim = None

    def fit(self, data, *, means_init=None, dim=None, ctx=None):
        """GMM.py:23-63.  `data`: (n,2) or (n,3) array, object with ``.points``, or a DeviceCloud (dim 3 unless `dim` says 2;
        nothing is downloaded).  Without `means_init` (k,dim) exactly one ``np.random.random((k, dim))`` is drawn, so the global
        stream ends where the reference's ``fit`` leaves it.  A singular component raises ``np.linalg.LinAlgError`` (attributes
        ``iteration``, ``component``) and leaves this object as it was."""
        cloud, dim, owned = _as_cloud(data, dim, ctx)
        try:
            k = int(self.n_clusters)
            p = L.GmmParams()
            L.lib().pcr_gmm_default_params(C.byref(p))
            p.n_clusters, p.dim, p.max_iter, p.tol = k, dim, int(self.max_iter), float(self.tol)
            if not (1 <= k <= L.PCR_GMM_MAX_K) or dim not in (2, 3) or p.max_iter < 1:
                raise L.PcrError(L.PCR_E_INVALID)
            if means_init is None:
                means0 = np.random.random((k, dim))   # GMM.py:25
            else:
                means0 = L.as_f64(means_init)
                if means0.shape != (k, dim):
                    raise ValueError(f"means_init: expected shape {(k, dim)}, got {means0.shape}")
            means, covs, weights = np.empty((k, dim)), np.empty((k, dim, dim)), np.empty(k)
            hist = np.empty(p.max_iter)
            res = L.GmmResult()
            st = L.lib().pcr_gmm_fit(cloud.ctx.handle, cloud.handle, C.byref(p), L.dptr(means0), L.dptr(means), L.dptr(covs), L.dptr(weights),
                                     L.dptr(hist), C.byref(res))
        finally:
            if owned:
                cloud.free()
        if st == L.PCR_E_SINGULAR:
            err = np.linalg.LinAlgError(
                f"GMM.fit: component {res.bad_component} has no points or a covariance that is not positive definite in iteration {res.bad_iter}")
            err.iteration, err.component = int(res.bad_iter), int(res.bad_component)
            raise err
        L.check(st, cloud.ctx.handle, soft=())
        self.means, self.covs, self.weights = means, covs, weights.reshape(k, 1)
        self.n_iter_ = int(res.iters)
        self.nll_ = float(res.nll)
        self.nll_history_ = hist[:res.iters].copy()
        self.converged_ = bool(res.converged)
        self.device_ms_ = float(res.device_ms)
        self._dim = dim
        return self

    def _predict(self, data, want_resp, ctx):
        if self.means is None:
            raise RuntimeError("GMM.predict before fit")
        cloud, dim, owned = _as_cloud(data, self._dim, ctx)
        try:
            k = int(self.n_clusters)
            labels = np.empty(cloud.n, dtype=np.int32)
            resp = np.empty((cloud.n, k)) if want_resp else None
            st = L.lib().pcr_gmm_predict(cloud.ctx.handle, cloud.handle, k, dim, L.dptr(L.as_f64(self.means)), L.dptr(L.as_f64(self.covs)),
                                         L.dptr(L.as_f64(self.weights).reshape(k)), L.iptr(labels), L.dptr(resp) if want_resp else None, None)
        finally:
            if owned:
                cloud.free()
        if st == L.PCR_E_SINGULAR:
            raise np.linalg.LinAlgError("GMM.predict: a covariance is not positive definite")
        L.check(st, cloud.ctx.handle, soft=())
        return labels, resp

    def predict(self, data, *, ctx=None):
        """GMM.py:65-70: the component of the largest weighted density per row (the lowest on ties), like ``np.argmax``."""
        return self._predict(data, False, ctx)[0].astype(np.intp)

    def predict_proba(self, data, *, ctx=None):
        """(n,k) responsibilities gamma of GMM.py:31-35 under the fitted parameters."""
        return self._predict(data, True, ctx)[1]
