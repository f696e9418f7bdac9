"""Host side of spectral clustering (include/pcr.h: pcr_spectral_*, pcr_knn_graph, pcr_sym_eig_jacobi): exported symbols, structs
and defaults; every argument check, which sits in front of the first use of the device (dummy handles are never dereferenced on those
paths; a hand-made block stands in for a cloud of n points where a check needs n); the host Jacobi solve against LAPACK; the NumPy
restatement of tests/spectral_checks.py against the golden recorded from the reference's own class; Python argument errors.  No GPU
needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import spectral_checks as sc
from tests.conftest import load_golden

NEW_SYMBOLS = ["pcr_spectral_default_params", "pcr_knn_graph", "pcr_spectral_embed", "pcr_spectral_fit", "pcr_sym_eig_jacobi"]
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pcr.h")
WIDTH = {"int32_t": 4, "int64_t": 8, "double": 8}


def _header_struct_size(name):
    """Size of a struct of int32_t / int64_t / double (arrays) fields as include/pcr.h declares it, natural alignment."""
    text = open(HEADER).read()
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", text, re.S).group(1)
    size = 0
    for typ, _, count in re.findall(r"^\s*(int32_t|int64_t|double)\s+(\w+)(?:\[(\d+)\])?;", body, re.M):
        width = WIDTH[typ]
        size = (size + width - 1) // width * width + width * int(count or 1)
    return (size + 7) // 8 * 8


def _fake_cloud(n):
    """The head of a cloud handle (records pointer, n) for the checks that read n and return before the device."""
    block = (C.c_uint64 * 32)()
    block[1] = n
    return block


def test_symbols_structs_and_defaults(pcp):
    L = pcp._lib
    lib = L.lib()
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES and hasattr(lib, name), name
    header = open(HEADER).read()
    assert re.search(r"#define PCR_SPECTRAL_MAX_K 8\b", header) and L.PCR_SPECTRAL_MAX_K == 8
    assert re.search(r"#define PCR_SPECTRAL_MAX_NNK 15\b", header) and L.PCR_SPECTRAL_MAX_NNK == 15
    assert C.sizeof(L.SpectralParams) == _header_struct_size("pcr_spectral_params") == 72
    assert C.sizeof(L.SpectralResult) == _header_struct_size("pcr_spectral_result") == 240
    p = L.SpectralParams()
    p.n_clusters = p.nnk = p.normalized = p.max_iter = p.kmeans_max_iter = p.reserved_i = -1
    p.tol = p.kmeans_tol = -1.0
    lib.pcr_spectral_default_params(C.byref(p))
    assert (p.n_clusters, p.nnk, p.normalized, p.max_iter, p.kmeans_max_iter, p.tol, p.kmeans_tol, p.reserved_i) == (2, 7, 1, 200, 300, 1e-8, 1e-4, 0)
    assert list(p.reserved) == [0.0] * 4
    lib.pcr_spectral_default_params(None)      # ignored
    m = pcp.spetral_clustering()
    assert (m.n_clusters, m.nnk_, m.normalized_) == (2, 7, True) and len(m.labels_) == 0      # spectral_clustering.py:8-12
    assert pcp.spectral_clustering is pcp.spetral_clustering
    assert len(pcp.spetral_clustering(n_clusters=3).predict()) == 0


def _fit(pcp, cloud, ctx=C.c_void_p(8), seeds=None, embed=True, **kw):
    L = pcp._lib
    p = L.SpectralParams()
    L.lib().pcr_spectral_default_params(C.byref(p))
    for name, v in kw.items():
        setattr(p, name, v)
    lab, emb, res = np.zeros(8, dtype=np.int32), np.zeros(64), L.SpectralResult()
    fit = L.lib().pcr_spectral_fit(ctx, cloud, C.byref(p), L.lptr(seeds) if seeds is not None else None, L.iptr(lab), L.dptr(emb), None, None, C.byref(res))
    return fit, L.lib().pcr_spectral_embed(ctx, cloud, C.byref(p), L.dptr(emb), C.byref(res)) if embed else None


def test_invalid_arguments_are_refused_before_the_device(pcp):
    L = pcp._lib
    lib = L.lib()
    dummy = C.c_void_p(8)
    for kw in ({"n_clusters": 0}, {"n_clusters": 9}, {"n_clusters": -1}, {"nnk": 0}, {"nnk": 16}, {"max_iter": 0}, {"max_iter": -3}, {"tol": 0.0}, {"tol": -1e-8},
               {"tol": np.nan}, {"tol": np.inf}, {"kmeans_max_iter": 0}, {"kmeans_tol": -1.0}, {"kmeans_tol": np.nan}):
        assert _fit(pcp, dummy, **kw) == (L.PCR_E_INVALID, L.PCR_E_INVALID), kw
    # NULL handles and required pointers
    p, res = L.SpectralParams(), L.SpectralResult()
    lib.pcr_spectral_default_params(C.byref(p))
    lab, emb = np.zeros(8, dtype=np.int32), np.zeros(64)
    full = [dummy, dummy, C.byref(p), None, L.iptr(lab), L.dptr(emb), None, None, C.byref(res)]
    for i in (0, 1, 2, 4, 8):
        args = list(full)
        args[i] = None
        assert lib.pcr_spectral_fit(*args) == L.PCR_E_INVALID, i
    full = [dummy, dummy, C.byref(p), L.dptr(emb), C.byref(res)]
    for i in range(5):
        args = list(full)
        args[i] = None
        assert lib.pcr_spectral_embed(*args) == L.PCR_E_INVALID, i
    indptr, idx, w = np.zeros(8, dtype=np.int64), np.zeros(8, dtype=np.int32), np.zeros(8)
    full = [dummy, dummy, 7, L.lptr(indptr), None, None, None]
    for i in (0, 1, 3):
        args = list(full)
        args[i] = None
        assert lib.pcr_knn_graph(*args) == L.PCR_E_INVALID, i
    assert lib.pcr_knn_graph(dummy, dummy, 7, L.lptr(indptr), L.iptr(idx), None, None) == L.PCR_E_INVALID      # indices without weights
    for nnk in (0, -1, 16):
        assert lib.pcr_knn_graph(dummy, dummy, nnk, L.lptr(indptr), L.iptr(idx), L.dptr(w), None) == L.PCR_E_INVALID
    a = np.eye(2)
    for args in ((0, L.dptr(a), L.dptr(w), L.dptr(emb)), (65, L.dptr(a), L.dptr(w), L.dptr(emb)), (2, None, L.dptr(w), L.dptr(emb)), (2, L.dptr(a), None, L.dptr(emb)),
                 (2, L.dptr(a), L.dptr(w), None)):
        assert lib.pcr_sym_eig_jacobi(*args) == L.PCR_E_INVALID


def test_cloud_size_and_seed_rows_are_refused_before_the_device(pcp):
    L = pcp._lib
    lib = L.lib()
    dummy = C.c_void_p(8)
    indptr = np.zeros(8, dtype=np.int64)
    blank = C.cast(_fake_cloud(0), C.c_void_p)
    assert lib.pcr_cloud_size(blank) == 0
    assert _fit(pcp, blank) == (L.PCR_E_EMPTY, L.PCR_E_EMPTY)
    assert _fit(pcp, blank, n_clusters=0) == (L.PCR_E_INVALID, L.PCR_E_INVALID)        # the argument checks come first
    assert lib.pcr_knn_graph(dummy, blank, 7, L.lptr(indptr), None, None, None) == L.PCR_E_EMPTY
    small = C.cast(_fake_cloud(8), C.c_void_p)      # n = nnk + 1: the reference raises IndexError
    assert lib.pcr_cloud_size(small) == 8
    assert _fit(pcp, small) == (L.PCR_E_INVALID, L.PCR_E_INVALID)
    assert lib.pcr_knn_graph(dummy, small, 7, L.lptr(indptr), None, None, None) == L.PCR_E_INVALID
    assert _fit(pcp, C.cast(_fake_cloud(5), C.c_void_p), nnk=3, n_clusters=6) == (L.PCR_E_INVALID, L.PCR_E_INVALID)     # more clusters than rows
    cloud = C.cast(_fake_cloud(100), C.c_void_p)
    for seeds in ([0, 100], [-1, 5], [7, 7]):
        assert _fit(pcp, cloud, seeds=np.array(seeds, dtype=np.int64), embed=False)[0] == L.PCR_E_INVALID, seeds
    assert _fit(pcp, cloud, seeds=np.array([3, 3, 4], dtype=np.int64), embed=False, n_clusters=3)[0] == L.PCR_E_INVALID


def _triple():
    rng = np.random.default_rng(5)
    q, _ = np.linalg.qr(rng.normal(size=(16, 16)))
    d = np.array([2.0, 2.0, 2.0] + list(np.linspace(-1, 1.5, 13)))
    return q @ np.diag(d) @ q.T


def _sym(n, seed):
    a = np.random.default_rng(seed).normal(size=(n, n))
    return a + a.T


@pytest.mark.parametrize("name,A", [("n1", np.array([[3.5]])), ("n2", _sym(2, 1)), ("n16", _sym(16, 2)), ("n64", _sym(64, 3)), ("triple", _triple()),
                                    ("diagonal", np.diag([3.0, -1.0, 2.0])), ("zero", np.zeros((4, 4)))])
def test_jacobi_against_lapack(pcp, name, A):
    L = pcp._lib
    n = len(A)
    A = np.ascontiguousarray(0.5 * (A + A.T))
    keep = A.copy()
    vals, vecs = np.empty(n), np.empty((n, n))
    assert L.lib().pcr_sym_eig_jacobi(n, L.dptr(A), L.dptr(vals), L.dptr(vecs)) == L.PCR_OK
    assert np.array_equal(A, keep)
    norm = max(np.linalg.norm(A, 2), 1e-300)
    ref = np.linalg.eigh(A)[0]
    print(name, "eigenvalues", np.abs(vals - ref).max() / norm, "orthogonality", np.abs(vecs.T @ vecs - np.eye(n)).max(),
          "residual", np.abs(A @ vecs - vecs * vals).max() / norm)
    assert (np.diff(vals) >= 0).all()
    assert np.abs(vals - ref).max() <= 1e-13 * norm
    assert np.abs(vecs.T @ vecs - np.eye(n)).max() <= 1e-12 * max(norm, 1.0) and np.abs(A @ vecs - vecs * vals).max() <= 1e-12 * norm


def _golden_data(g, name):
    args = g[name + "_args"]
    return sc.bridge(int(args[0]), int(args[1])) if name == "bridge" else sc.blobs_even(int(args[0]), int(args[1]))


@pytest.mark.parametrize("name", ["bridge", "blobs_norm", "blobs_raw"])
def test_restatement_reproduces_the_reference(name):
    g = load_golden("spectral.npz")
    assert name in list(g["cases"])
    data, k, normalized = _golden_data(g, name), int(g[name + "_k"]), bool(g[name + "_normalized"])
    r = sc.fit(data, k, nnk=7, normalized=normalized)
    assert r["graph"]["tie_gap"] > 1e-9 and r["graph"]["min_dist"] > 0
    assert np.abs(r["lam"] - g[name + "_eigenvalues"]).max() <= 1e-10
    assert sc.same_partition(r["labels"], g[name + "_labels"])
    if name == "bridge":      # connected: the Fiedler vector is defined up to its sign
        assert abs(r["lam"][1] - 2.55e-3) < 1e-5 and abs(r["lam"][2] - 1.36e-2) < 1e-4
        V = g[name + "_V"]
        for j in range(k):
            ref = V[:, j] * np.sign(V[np.argmax(np.abs(V[:, j])), j])
            assert np.abs(r["embedding"][:, j] - ref).max() <= 1e-8, j
    else:
        import scipy.sparse.csgraph as csg
        n_comp, comp = csg.connected_components(sc.csr(r["graph"]), directed=False)
        assert n_comp == 3 and sc.same_partition(comp, g[name + "_labels"])
        assert len(set(comp[r["seed_rows"]])) == 3


def test_circles_golden_records_the_reference_failure():
    g = load_golden("spectral.npz")
    assert str(g["circles_reference_raises"]) == "ValueError: Complex data not supported"
    X, y = sc.circles(*[t(v) for t, v in zip((int, float, float, int), g["circles_args"])])
    r = sc.fit(X, 2)
    assert np.isrealobj(r["embedding"]) and sc.same_partition(r["labels"], y)


def test_restatement_rules():
    """A self-test of the yardstick: sign rule, maximin ties, self dropped by id, mutual pairs kept once."""
    U = np.array([[0.5, -0.1], [-0.5, 0.7], [0.5, -0.7], [0.5, 0.1]])
    E = sc.embedding(U, np.ones(4), 2, False)
    assert E[0, 0] > 0 and E[1, 1] > 0 and np.allclose((E * E).sum(axis=0), 1.0)
    assert list(sc.maximin(np.array([[0.0], [1.0], [-1.0], [0.5]]), 3)) == [0, 1, 2]
    pts = np.array([[0.0, 0, 0], [1.0, 0, 0], [3.0, 0, 0], [7.0, 0, 0]])
    g = sc.graph(pts, 1)
    assert list(g["indptr"]) == [0, 1, 3, 5, 6] and list(g["indices"]) == [1, 0, 2, 1, 3, 2] and np.array_equal(g["weights"], [1, 1, .5, .5, .25, .25])


def test_python_argument_errors(pcp):
    L = pcp._lib
    pts = np.zeros((100, 3))
    for kw, fit_kw in (({"n_clusters": 0}, {}), ({"n_clusters": 9}, {}), ({"nnk": 0}, {}), ({"nnk": 16}, {}), ({}, {"max_iter": 0}), ({}, {"tol": 0.0}), ({}, {"tol": np.nan})):
        with pytest.raises(L.PcrError) as e:
            pcp.spetral_clustering(**kw).fit(pts, **fit_kw)
        assert e.value.status == L.PCR_E_INVALID
    with pytest.raises(L.PcrError) as e:
        pcp.spetral_clustering().fit(np.zeros((10, 4)))
    assert e.value.status == L.PCR_E_INVALID
    with pytest.raises(L.PcrError) as e:
        pcp.spetral_clustering().fit(np.zeros((0, 3)))
    assert e.value.status == L.PCR_E_EMPTY
    for seeds in ([0], [0, 1, 2], [[0, 1]]):
        with pytest.raises(ValueError):
            pcp.spetral_clustering(2).fit(pts, seed_rows=seeds)
    with pytest.raises(L.PcrError) as e:
        pcp.knn_graph(pts, nnk=16)
    assert e.value.status == L.PCR_E_INVALID
