"""Host side of the Gaussian mixture (Cluster_KMeans_GMM/GMM.py:13-71): exported symbols, structs and defaults; the two NumPy
restatements of tests/gmm_checks.py against the golden recorded from the reference's own class; pcr_gmm_log_density -- the
__host__ __device__ function the kernels call -- against scipy; argument validation.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from tests import gmm_checks
from tests.conftest import load_golden

NEW_SYMBOLS = ["pcr_gmm_default_params", "pcr_gmm_fit", "pcr_gmm_step", "pcr_gmm_predict", "pcr_gmm_log_density"]


def _log_density(pcp, x, mean, cov, w):
    L = pcp._lib
    x, mean, cov = (np.ascontiguousarray(v, dtype=np.float64) for v in (x, mean, cov))
    a = C.c_double(np.nan)
    st = L.lib().pcr_gmm_log_density(len(x), L.dptr(x), L.dptr(mean), L.dptr(cov), float(w), C.byref(a))
    return st, a.value


def test_symbols_structs_and_defaults(pcp):
    L = pcp._lib
    lib = L.lib()
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert L.PCR_E_SINGULAR == -8 and L.PCR_GMM_MAX_K == 32
    assert b"singular" in lib.pcr_strerror(L.PCR_E_SINGULAR)
    assert C.sizeof(L.GmmParams) == 56 and C.sizeof(L.GmmResult) == 72   # include/pcr.h, natural alignment
    p = L.GmmParams()
    p.n_clusters, p.dim, p.max_iter, p.reserved_i, p.tol = -1, -1, -1, -1, -1.0
    lib.pcr_gmm_default_params(C.byref(p))
    assert (p.dim, p.max_iter, p.tol, p.reserved_i) == (3, 50, 0.001, 0) and list(p.reserved) == [0.0] * 4
    m = pcp.GMM(n_clusters=3)
    assert (m.n_clusters, m.max_iter, m.tol) == (3, 50, 0.001)              # GMM.py:14
    assert m.means is None and m.covs is None and np.array_equal(m.weights, np.ones((3, 1)) / 3)   # GMM.py:18-20


def test_restatements_reproduce_the_reference():
    g = load_golden("gmm.npz")
    assert int(g["n_iter"]) == 46 and g["data"].shape == (2000, 2)
    assert np.array_equal(g["data"], gmm_checks.toy_data(int(g["data_seed"])))
    np.random.seed(int(g["np_random_seed"]))
    assert np.array_equal(np.random.random((3, 2)), g["means_init"])       # GMM.py:25 is the first draw of fit
    for fit in (gmm_checks.fit_literal, gmm_checks.fit_log):
        r = fit(g["data"], g["means_init"], int(g["max_iter"]), float(g["tol"]))
        assert r["n_iter"] == int(g["n_iter"]), fit.__name__
        for key in ("means", "covs", "weights"):
            assert r[key].shape == g[key].shape and np.abs(r[key] - g[key]).max() <= 1e-12, (fit.__name__, key)
        assert np.allclose(r["nll_history"], g["nll_history"], rtol=1e-12, atol=0)
    labels, gap = gmm_checks.predict_log(g["data"], g["means"], g["covs"], g["weights"])
    clear = gap > 1e-9
    assert clear.mean() >= 0.99 and np.array_equal(labels[clear], g["labels"][clear])
    # the condition the generator asserts: no step within 1e-6 of tol
    h = np.concatenate([[np.inf], g["nll_history"]])
    assert np.abs((h[:-1] - h[1:]) - float(g["tol"])).min() > 1e-6


def test_literal_restatement_fails_at_lidar_scale():
    """What the log domain is for: the reference's densities underflow to 0/0 on data ~40 m from its [0,1) means."""
    pts = gmm_checks.lidar_blobs()
    np.random.seed(0)
    with pytest.raises((ValueError, np.linalg.LinAlgError)):
        gmm_checks.fit_literal(pts, np.random.random((3, 3)))
    r = gmm_checks.fit_log(pts, pts[:3].copy())
    assert np.isfinite(r["means"]).all() and r["n_iter"] >= 1


@pytest.mark.parametrize("dim", [2, 3])
def test_log_density_against_scipy(pcp, dim):
    """a = log w + logpdf to 1e-12 max(1, |a|) for well-conditioned random covariances (condition number <= ~30: the error of the
    Mahalanobis term grows with it on both sides), |a| up to ~700."""
    from scipy.stats import multivariate_normal

    L = pcp._lib
    rng = np.random.default_rng(40 + dim)
    biggest = 0.0
    for case in range(300):
        q, _ = np.linalg.qr(rng.normal(size=(dim, dim)))
        ev = rng.uniform(0.2, 5.0, size=dim) * 10.0 ** rng.integers(-2, 3)
        cov = (q * ev) @ q.T
        cov = 0.5 * (cov + cov.T)
        mean = rng.normal(size=dim) * 50.0
        w = float(rng.uniform(1e-6, 1.0))
        r = [0.0, 1.0, 5.0, 20.0, 37.0][case % 5]       # Mahalanobis radius: |a| ~ r^2 / 2
        u = rng.normal(size=dim)
        x = mean + np.linalg.cholesky(cov) @ (r * u / np.linalg.norm(u))
        want = multivariate_normal.logpdf(x, mean=mean, cov=cov) + np.log(w)
        st, a = _log_density(pcp, x, mean, cov, w)
        assert st == L.PCR_OK
        assert abs(a - want) <= 1e-12 * max(1.0, abs(want)), (case, a, want)
        biggest = max(biggest, abs(want))
    assert biggest > 650.0


def test_log_density_singular_and_invalid(pcp):
    L = pcp._lib
    x3, m3 = np.array([1.0, 2.0, 3.0]), np.zeros(3)
    singular = [np.zeros((3, 3)), np.ones((3, 3)), np.diag([1.0, 1.0, 0.0]), np.array([[1.0, 2.0, 0], [2.0, 4.0, 0], [0, 0, 1.0]])]
    indefinite = [np.diag([1.0, -1.0, 1.0]), np.array([[1.0, 2.0, 0], [2.0, 1.0, 0], [0, 0, 1.0]]), np.diag([1.0, 1.0, np.nan]), np.diag([np.inf, 1.0, 1.0])]
    for cov in singular + indefinite:
        assert _log_density(pcp, x3, m3, cov, 0.5)[0] == L.PCR_E_SINGULAR, cov
    for cov in (np.zeros((2, 2)), np.array([[1.0, 1.0], [1.0, 1.0]]), np.array([[1.0, 3.0], [3.0, 1.0]])):
        assert _log_density(pcp, x3[:2], m3[:2], cov, 0.5)[0] == L.PCR_E_SINGULAR, cov
    assert _log_density(pcp, x3, m3, np.eye(3), 0.5)[0] == L.PCR_OK
    # dim 2 never looks at a third coordinate
    assert _log_density(pcp, x3[:2], m3[:2], np.eye(2), 0.5) == (L.PCR_OK, np.log(0.5) - np.log(2 * np.pi) - 2.5)
    f = L.lib().pcr_gmm_log_density
    a = C.c_double()
    e3 = np.eye(3)
    for dim in (1, 4, 0, -3):
        assert f(dim, L.dptr(x3), L.dptr(m3), L.dptr(e3), 0.5, C.byref(a)) == L.PCR_E_INVALID
    for w in (0.0, -0.5, np.nan, np.inf):
        assert f(3, L.dptr(x3), L.dptr(m3), L.dptr(e3), w, C.byref(a)) == L.PCR_E_INVALID
    assert f(3, None, L.dptr(m3), L.dptr(e3), 0.5, C.byref(a)) == L.PCR_E_INVALID
    assert f(3, L.dptr(x3), L.dptr(m3), L.dptr(e3), 0.5, None) == L.PCR_E_INVALID


def test_shape_limits_are_refused_before_the_device(pcp):
    """k in {0, 33}, dim in {1, 4}, max_iter 0 -> PCR_E_INVALID; the check sits in front of every use of the context (a non-NULL
    dummy handle is never dereferenced on these paths)."""
    L = pcp._lib
    lib = L.lib()
    dummy = C.c_void_p(8)
    buf = np.zeros(33 * 16)
    lab = np.zeros(4, dtype=np.int32)
    res = L.GmmResult()
    for k, dim, max_iter in ((0, 3, 50), (33, 3, 50), (3, 1, 50), (3, 4, 50), (3, 3, 0), (-1, 2, 50)):
        p = L.GmmParams()
        lib.pcr_gmm_default_params(C.byref(p))
        p.n_clusters, p.dim, p.max_iter = k, dim, max_iter
        assert lib.pcr_gmm_fit(dummy, dummy, C.byref(p), L.dptr(buf), L.dptr(buf), L.dptr(buf), L.dptr(buf), None, C.byref(res)) == L.PCR_E_INVALID
        if max_iter > 0:
            assert lib.pcr_gmm_step(dummy, dummy, k, dim, L.dptr(buf), L.dptr(buf), L.dptr(buf), None, None, None, None, None) == L.PCR_E_INVALID
            assert lib.pcr_gmm_predict(dummy, dummy, k, dim, L.dptr(buf), L.dptr(buf), L.dptr(buf), L.iptr(lab), None, None) == L.PCR_E_INVALID
    p = L.GmmParams()
    lib.pcr_gmm_default_params(C.byref(p))
    assert lib.pcr_gmm_fit(None, None, C.byref(p), L.dptr(buf), None, None, None, None, C.byref(res)) == L.PCR_E_INVALID
    with pytest.raises(L.PcrError) as e:
        pcp.GMM(3).fit(np.zeros((10, 4)))
    assert e.value.status == L.PCR_E_INVALID
    with pytest.raises(L.PcrError) as e:
        pcp.GMM(3).fit(np.zeros((0, 3)))
    assert e.value.status == L.PCR_E_EMPTY
