"""Spectral clustering: class spetral_clustering of Cluster_KMeans_GMM/spectral_clustering.py:7-46 (same constructor and spelling,
``fit`` / ``predict``) with the k-NN graph, the Laplacian's eigenvectors and the K-Means on the embedding on the device
(include/pcr.h: pcr_spectral_fit, pcr_knn_graph).

Stated deviations: the eigenpairs are those of the symmetric ``I - D^-1/2 W D^-1/2`` (similar to the reference's
``D^-1 L``), so they are real on every input -- the reference's ``LA.eig`` returns complex pairs on some and then raises --; the
K-Means on the embedding is Lloyd's iteration from maximin seeds (or the caller's ``seed_rows``) instead of scikit-learn's
k-means++ with restarts on the global RNG, so ``fit`` is repeatable and does not touch ``np.random``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .gmm import _as_cloud

__all__ = ["spetral_clustering", "spectral_clustering", "knn_graph"]


def knn_graph(data, nnk=7, *, ctx=None):
    """The symmetrised k-NN graph of spectral_clustering.py:17-30 as a CSR by caller row -> (indptr int64 (n+1,), indices int32,
    weights = 1 / dist), columns ascending.  Two distinct rows at distance 0: ``PcrError`` (PCR_E_SINGULAR, attribute ``bad_row``)."""
    nnk = int(nnk)
    if not (1 <= nnk <= L.PCR_SPECTRAL_MAX_NNK):
        raise L.PcrError(L.PCR_E_INVALID, f"nnk {nnk} (1..{L.PCR_SPECTRAL_MAX_NNK})")
    cloud, _, owned = _as_cloud(data, None, ctx)
    try:
        indptr = np.empty(cloud.n + 1, dtype=np.int64)
        bad = C.c_int32(-1)
        st = L.lib().pcr_knn_graph(cloud.ctx.handle, cloud.handle, nnk, L.lptr(indptr), None, None, C.byref(bad))
        _check(st, cloud, bad.value)
        indices, weights = np.empty(indptr[-1], dtype=np.int32), np.empty(indptr[-1])
        st = L.lib().pcr_knn_graph(cloud.ctx.handle, cloud.handle, nnk, L.lptr(indptr), L.iptr(indices), L.dptr(weights), C.byref(bad))
        _check(st, cloud, bad.value)
    finally:
        if owned:
            cloud.free()
    return indptr, indices, weights


def _check(st, cloud, bad_row):
    try:
        L.check(st, cloud.ctx.handle, soft=())
    except L.PcrError as e:
        e.bad_row = int(bad_row)
        raise


class spetral_clustering(object):
    """spectral_clustering.py:7-12.  After ``fit``: ``labels_`` (n,) intp by caller row, ``embedding_`` (n,k), ``eigenvalues_`` (k,)
    ascending, ``residuals_`` (k,), ``next_eigenvalue_`` (the gap behind the last wanted one), ``n_iter_``, ``converged_``,
    ``n_edges_``, ``max_degree_``, ``seed_rows_`` (k,), ``centers_`` (k,k), ``device_ms_`` (dict: graph, solver, kmeans)."""

    def __init__(self, n_clusters=2, nnk=7, normalized=True):
        self.n_clusters = n_clusters
        self.nnk_ = nnk
        self.labels_ = np.empty(0)
        self.normalized_ = normalized

        self.embedding_ = None
        self.eigenvalues_ = None
        self.residuals_ = None
        self.next_eigenvalue_ = None
        self.n_iter_ = 0
        self.converged_ = False
        self.n_edges_ = 0
        self.max_degree_ = 0
        self.seed_rows_ = None
        self.centers_ = None
        self.n_spmm_ = 0
        self.device_ms_ = None

    def fit(self, data, *, seed_rows=None, tol=1e-8, max_iter=200, ctx=None):
        """spectral_clustering.py:15-43.  `data`: (n,2) or (n,3) array, object with ``.points``, or a DeviceCloud (nothing is
        downloaded but the results).  `seed_rows`: k distinct caller rows whose embedding rows seed the K-Means (default: maximin
        from row 0).  `tol`, `max_iter`: of the eigensolver (residuals <= 2 tol).  n_clusters outside 1..8, nnk outside 1..15,
        max_iter < 1, a tol that is not positive and finite, fewer than nnk + 2 points: ``PcrError`` (PCR_E_INVALID), the first four
        before anything is uploaded; two distinct rows at distance 0: ``PcrError`` (PCR_E_SINGULAR) with ``bad_row``."""
        k, nnk, max_iter, tol = int(self.n_clusters), int(self.nnk_), int(max_iter), float(tol)
        if not (1 <= k <= L.PCR_SPECTRAL_MAX_K) or not (1 <= nnk <= L.PCR_SPECTRAL_MAX_NNK) or max_iter < 1 or not (np.isfinite(tol) and tol > 0):
            raise L.PcrError(L.PCR_E_INVALID, f"n_clusters {k} (1..{L.PCR_SPECTRAL_MAX_K}), nnk {nnk} (1..{L.PCR_SPECTRAL_MAX_NNK}), max_iter {max_iter} (>= 1), tol {tol} (> 0)")
        if seed_rows is not None:
            seed_rows = np.ascontiguousarray(seed_rows, dtype=np.int64)
            if seed_rows.shape != (k,):
                raise ValueError(f"seed_rows: expected shape {(k,)}, got {seed_rows.shape}")
        cloud, _, owned = _as_cloud(data, None, ctx)
        try:
            n = cloud.n
            p = L.SpectralParams()
            L.lib().pcr_spectral_default_params(C.byref(p))
            p.n_clusters, p.nnk, p.normalized, p.max_iter, p.tol = k, nnk, 1 if self.normalized_ else 0, max_iter, tol
            lab, emb = np.empty(n, dtype=np.int32), np.empty((n, k))
            centers, seeds = np.empty((k, k)), np.empty(k, dtype=np.int64)
            res = L.SpectralResult()
            st = L.lib().pcr_spectral_fit(cloud.ctx.handle, cloud.handle, C.byref(p), L.lptr(seed_rows) if seed_rows is not None else None,
                                          L.iptr(lab), L.dptr(emb), L.dptr(centers), L.lptr(seeds), C.byref(res))
            _check(st, cloud, res.bad_row)
        finally:
            if owned:
                cloud.free()
        self.labels_ = lab.astype(np.intp)
        self.embedding_ = emb
        self.eigenvalues_ = np.array(res.eigenvalues[:k])
        self.residuals_ = np.array(res.residuals[:k])
        self.next_eigenvalue_ = float(res.next_eigenvalue)
        self.n_iter_ = int(res.iters)
        self.n_spmm_ = int(res.spmm)
        self.converged_ = bool(res.converged)
        self.n_edges_ = int(res.n_edges)
        self.max_degree_ = int(res.max_degree)
        self.seed_rows_ = seeds
        self.centers_ = centers
        self.kmeans_iter_ = int(res.kmeans_iters)
        self.kmeans_converged_ = bool(res.kmeans_converged)
        self.inertia_ = float(res.inertia)
        self.device_ms_ = {"graph": float(res.graph_ms), "solver": float(res.solver_ms), "kmeans": float(res.kmeans_ms)}
        return self

    def predict(self):
        """spectral_clustering.py:45-46: the labels of the fitted data."""
        return self.labels_

    def fit_predict(self, data, *, seed_rows=None, tol=1e-8, max_iter=200, ctx=None):
        return self.fit(data, seed_rows=seed_rows, tol=tol, max_iter=max_iter, ctx=ctx).labels_


spectral_clustering = spetral_clustering
