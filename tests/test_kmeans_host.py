"""Host side of K-Means (include/pcr.h: pcr_kmeans_*, pcr_cloud_download_rows): exported symbols, structs and defaults; every
argument check, which sits in front of the first use of the device (dummy handles are never dereferenced on those paths); the NumPy
restatement of tests/kmeans_checks.py against the golden recorded from scikit-learn's Lloyd; Python argument errors.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import gmm_checks, kmeans_checks
from tests.conftest import load_golden

NEW_SYMBOLS = ["pcr_kmeans_default_params", "pcr_kmeans_fit", "pcr_kmeans_step", "pcr_kmeans_predict", "pcr_cloud_download_rows"]
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pcr.h")


def _header_struct_size(name):
    """Size of a struct of int32_t / double (arrays) fields as include/pcr.h declares it, natural alignment."""
    text = open(HEADER).read()
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", text, re.S).group(1)
    size = 0
    for typ, _, count in re.findall(r"^\s*(int32_t|double)\s+(\w+)(?:\[(\d+)\])?;", body, re.M):
        width = 4 if typ == "int32_t" else 8
        size = (size + width - 1) // width * width + width * int(count or 1)
    return (size + 7) // 8 * 8


def test_symbols_structs_and_defaults(pcp):
    L = pcp._lib
    lib = L.lib()
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES and hasattr(lib, name), name
    header = open(HEADER).read()
    assert re.search(r"#define PCR_KMEANS_MAX_K 32\b", header) and L.PCR_KMEANS_MAX_K == 32 == L.PCR_GMM_MAX_K
    assert C.sizeof(L.KmeansParams) == _header_struct_size("pcr_kmeans_params") == 56
    assert C.sizeof(L.KmeansResult) == _header_struct_size("pcr_kmeans_result") == 72
    p = L.KmeansParams()
    p.n_clusters, p.dim, p.max_iter, p.reserved_i, p.tol = -1, -1, -1, -1, -1.0
    lib.pcr_kmeans_default_params(C.byref(p))
    assert (p.n_clusters, p.dim, p.max_iter, p.tol, p.reserved_i) == (2, 3, 300, 1e-4, 0) and list(p.reserved) == [0.0] * 4
    lib.pcr_kmeans_default_params(None)      # ignored
    m = pcp.K_Means()
    assert (m.n_clusters, m.tolerance, m.max_iter) == (2, 0.0001, 300)
    assert pcp.K_Means(n_clusters=5).n_clusters == 5        # compare_cluster.py:105
    assert m.centers_ is None and m.labels_ is None and m.n_iter_ == 0 and not m.converged_


def _calls(pcp, cloud):
    """fit / step / predict with every pointer given, as closures over (k, dim, max_iter, tol, centres)."""
    L = pcp._lib
    lib = L.lib()
    dummy = C.c_void_p(8)
    out = np.zeros(33 * 3)
    cnt = np.zeros(33, dtype=np.int64)
    lab = np.zeros(4, dtype=np.int32)
    res = L.KmeansResult()

    def fit(k, dim, max_iter, tol, c):
        p = L.KmeansParams()
        lib.pcr_kmeans_default_params(C.byref(p))
        p.n_clusters, p.dim, p.max_iter, p.tol = k, dim, max_iter, tol
        return lib.pcr_kmeans_fit(dummy, cloud, C.byref(p), L.dptr(c), L.dptr(out), L.lptr(cnt), L.iptr(lab), None, None, C.byref(res))

    def step(k, dim, c):
        return lib.pcr_kmeans_step(dummy, cloud, k, dim, L.dptr(c), L.dptr(out), L.lptr(cnt), None, None, None)

    def predict(k, dim, c):
        return lib.pcr_kmeans_predict(dummy, cloud, k, dim, L.dptr(c), L.iptr(lab), None, None)

    return fit, step, predict


def test_invalid_arguments_are_refused_before_the_device(pcp):
    L = pcp._lib
    lib = L.lib()
    dummy = C.c_void_p(8)
    fit, step, predict = _calls(pcp, dummy)
    good = np.ones(33 * 3)
    for k, dim, max_iter, tol in ((0, 3, 300, 1e-4), (33, 3, 300, 1e-4), (-1, 2, 300, 1e-4), (3, 1, 300, 1e-4), (3, 4, 300, 1e-4), (3, 3, 0, 1e-4),
                                  (3, 3, -5, 1e-4), (3, 3, 300, -1e-9), (3, 3, 300, np.nan), (3, 3, 300, np.inf), (3, 3, 300, -np.inf)):
        assert fit(k, dim, max_iter, tol, good) == L.PCR_E_INVALID, (k, dim, max_iter, tol)
    for k, dim in ((0, 3), (33, 3), (-1, 2), (3, 1), (3, 4)):
        assert step(k, dim, good) == L.PCR_E_INVALID and predict(k, dim, good) == L.PCR_E_INVALID, (k, dim)
    for bad_value in (np.nan, np.inf, -np.inf):
        for dim in (2, 3):
            bad = np.ones(33 * 3)
            bad[3 * dim - 1] = bad_value            # the last entry of (k, dim) = (3, dim)
            assert fit(3, dim, 300, 1e-4, bad) == L.PCR_E_INVALID
            assert step(3, dim, bad) == L.PCR_E_INVALID and predict(3, dim, bad) == L.PCR_E_INVALID
    # NULL handles and pointers
    p, res = L.KmeansParams(), L.KmeansResult()
    lib.pcr_kmeans_default_params(C.byref(p))
    out, cnt, lab = np.zeros(99), np.zeros(33, dtype=np.int64), np.zeros(4, dtype=np.int32)
    full = [dummy, dummy, C.byref(p), L.dptr(good), L.dptr(out), L.lptr(cnt), L.iptr(lab), None, None, C.byref(res)]
    for i in (0, 1, 2, 3, 4, 5, 9):
        args = list(full)
        args[i] = None
        assert lib.pcr_kmeans_fit(*args) == L.PCR_E_INVALID, i
    full = [dummy, dummy, 2, 3, L.dptr(good), None, None, None, None, None]
    for i in (0, 1, 4):
        args = list(full)
        args[i] = None
        assert lib.pcr_kmeans_step(*args) == L.PCR_E_INVALID, i
    full = [dummy, dummy, 2, 3, L.dptr(good), L.iptr(lab), None, None]
    for i in (0, 1, 4, 5):
        args = list(full)
        args[i] = None
        assert lib.pcr_kmeans_predict(*args) == L.PCR_E_INVALID, i
    rows = np.zeros(4, dtype=np.int64)
    full = [dummy, dummy, L.lptr(rows), 1, L.dptr(out)]
    for i in (0, 1, 2, 4):
        args = list(full)
        args[i] = None
        assert lib.pcr_cloud_download_rows(*args) == L.PCR_E_INVALID, i
    for m in (-1, 4097):
        assert lib.pcr_cloud_download_rows(dummy, dummy, L.lptr(rows), m, L.dptr(out)) == L.PCR_E_INVALID


def test_empty_cloud_is_refused_before_the_device(pcp):
    """A cloud of no points: a zeroed block stands in for the handle (no records, n = 0); the context is a dummy."""
    L = pcp._lib
    blank = (C.c_uint64 * 32)()
    fit, step, predict = _calls(pcp, C.cast(blank, C.c_void_p))
    good = np.ones(33 * 3)
    assert L.lib().pcr_cloud_size(C.cast(blank, C.c_void_p)) == 0
    assert fit(3, 3, 300, 1e-4, good) == L.PCR_E_EMPTY
    assert step(3, 3, good) == L.PCR_E_EMPTY and predict(3, 2, good) == L.PCR_E_EMPTY
    assert fit(0, 3, 300, 1e-4, good) == L.PCR_E_INVALID          # the argument checks come first
    rows = np.zeros(1, dtype=np.int64)
    assert L.lib().pcr_cloud_download_rows(C.c_void_p(8), C.cast(blank, C.c_void_p), L.lptr(rows), 1, L.dptr(good)) == L.PCR_E_INVALID   # row 0 of 0


def _golden_case(g, name):
    data = g["toy_data"] if name.startswith("toy") else kmeans_checks.blobs(*[int(v) for v in g["lidar_blobs_args"][:2]], lidar=bool(g["lidar_blobs_args"][2]))
    return data, int(g[name + "_k"])


@pytest.mark.parametrize("name", ["toy_k3", "lidar_k3", "lidar_k8"])
def test_restatement_reproduces_scikit_learn(name):
    g = load_golden("kmeans.npz")
    assert name in list(g["cases"])
    data, k = _golden_case(g, name)
    if name.startswith("toy"):
        assert data.shape == (2000, 2) and np.array_equal(data, gmm_checks.toy_data(int(g["toy_data_seed"])))
    else:
        assert data.shape == (20000, 3)
    np.random.seed(int(g["np_random_seed"]))
    rows = np.random.choice(len(data), k, replace=False)       # the default draw of K_Means.fit
    assert np.array_equal(rows, g[name + "_rows"]) and np.array_equal(data[rows], g[name + "_centers_init"])
    r = kmeans_checks.fit(data, g[name + "_centers_init"], max_iter=300, tol=0.0)
    assert r["converged"] and r["n_iter"] == int(g[name + "_n_iter"]) and r["n_empty"] == 0
    assert np.array_equal(r["labels"], g[name + "_labels"])
    assert np.abs(r["centers"] - g[name + "_centers"]).max() <= 1e-10
    assert abs(r["inertia"] - float(g[name + "_inertia"])) <= 1e-12 * float(g[name + "_inertia"])
    assert r["shift_history"][-1] == 0.0 and (r["shift_history"][:-1] > 0).all()
    # the conditions the generator asserts: no assignment and no stop that rounding could flip
    assert r["min_gap"].min() > 1e-9
    assert (np.abs(r["shift_history"] - 1e-4) > 1e-6 * 1e-4).all()


def test_restatement_rules():
    """A self-test of the yardstick, not of the library (it passes without it): the rules the scikit-learn golden does not show --
    ties to the lowest cluster, an empty cluster keeps its centre, the inclusive stop rule -- hold in tests/kmeans_checks.py, which
    the GPU tests compare the device against on exactly these cases."""
    pts = np.tile([[1.0, 2.0, 4.0]], (5, 1))
    s = kmeans_checks.step(pts, np.tile([[1.0, 2.0, 4.0]], (3, 1)))
    assert np.array_equal(s["labels"], np.zeros(5)) and list(s["counts"]) == [5, 0, 0] and s["n_empty"] == 2 and s["shift"] == 0.0
    assert np.array_equal(s["centers"], np.tile([[1.0, 2.0, 4.0]], (3, 1))) and s["inertia"] == 0.0
    far = np.array([[0.0, 0.0], [100.0, 100.0]])
    s = kmeans_checks.step(np.array([[0.0, 1.0], [0.0, 3.0]]), far)
    assert np.array_equal(s["centers"], [[0.0, 2.0], [100.0, 100.0]]) and s["shift"] == 2.0 and s["inertia"] == 10.0 and s["n_empty"] == 1
    r = kmeans_checks.fit(np.array([[0.0, 1.0], [0.0, 3.0]]), far, max_iter=1, tol=0.0)
    assert r["n_iter"] == 1 and not r["converged"]
    r = kmeans_checks.fit(np.array([[0.0, 1.0], [0.0, 3.0]]), far, max_iter=1, tol=2.0)
    assert r["n_iter"] == 1 and r["converged"]            # shift <= tol, inclusive


def test_python_argument_errors(pcp):
    L = pcp._lib
    with pytest.raises(L.PcrError) as e:
        pcp.K_Means(3).fit(np.zeros((10, 4)))
    assert e.value.status == L.PCR_E_INVALID
    with pytest.raises(L.PcrError) as e:
        pcp.K_Means(3).fit(np.zeros((0, 3)))
    assert e.value.status == L.PCR_E_EMPTY
    for shape in ((2, 3), (3, 2), (3,), (3, 3, 1)):
        with pytest.raises(ValueError):
            pcp.K_Means(3).fit(np.zeros((10, 3)), centers_init=np.zeros(shape))
    with pytest.raises(ValueError):
        pcp.K_Means(3).fit(np.zeros((10, 2)), centers_init=np.zeros((3, 3)))
    with pytest.raises(RuntimeError):
        pcp.K_Means(3).predict(np.zeros((10, 3)))
    # the ranges of n_clusters and max_iter, before anything is uploaded
    for kw in ({"n_clusters": 0}, {"n_clusters": 33}, {"n_clusters": 3, "max_iter": 0}):
        with pytest.raises(L.PcrError) as e:
            pcp.K_Means(**kw).fit(np.zeros((100, 3)))
        assert e.value.status == L.PCR_E_INVALID
    # the default draw needs k distinct rows; the global stream is left alone
    np.random.seed(9)
    state = np.random.get_state()
    with pytest.raises(ValueError, match="distinct seed rows"):
        pcp.K_Means(3).fit(np.zeros((2, 3)))
    assert np.array_equal(np.random.get_state()[1], state[1]) and np.random.get_state()[2] == state[2]
