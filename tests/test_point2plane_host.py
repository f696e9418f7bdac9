"""Host side of the point-to-plane refinement (Registration/main.py:87-95): exported symbols, default parameters and the
6x6 LDL^T update pcr_point2plane_solve, which runs the routine the kernel's finishing lane runs.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

NEW_SYMBOLS = ["pcr_index_set_normals", "pcr_index_has_normals", "pcr_icp_plane_default_params", "pcr_icp_point2plane",
               "pcr_point2plane_moments", "pcr_point2plane_solve"]


def _system(n_corr, seed, equal_normals=None):
    """A = sum J J^T, b = sum J r over seeded random correspondences, J = [s x n, n]."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(-10.0, 10.0, (n_corr, 3))
    if equal_normals is None:
        n = rng.normal(size=(n_corr, 3))
        n /= np.linalg.norm(n, axis=1, keepdims=True)
    else:
        n = np.tile(np.asarray(equal_normals, dtype=np.float64), (n_corr, 1))
    r = rng.normal(scale=0.1, size=n_corr)
    J = np.concatenate([np.cross(s, n), n], axis=1)
    return J.T @ J, J.T @ r


def _solve(pcp, A, b):
    L = pcp._lib
    Au = np.ascontiguousarray(A[np.triu_indices(6)])
    bc = np.ascontiguousarray(b, dtype=np.float64)
    x, U = np.full(6, np.nan), np.full(16, np.nan)
    st = L.lib().pcr_point2plane_solve(L.dptr(Au), L.dptr(bc), L.dptr(x), L.dptr(U))
    return st, x, U.reshape(4, 4)


def test_new_symbols_exported_with_signatures(pcp):
    L = pcp._lib
    lib = L.lib()
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES, name
        assert hasattr(lib, name), name
    for name in ("ICPConvergenceCriteria", "TransformationEstimationPointToPlane", "registration_icp", "refine_registration",
                 "icp_point2plane_device"):
        assert hasattr(pcp, name), name


def test_default_params(pcp):
    L = pcp._lib
    p = L.IcpPlaneParams()
    p.max_iter, p.rel_fitness, p.rel_rmse = -1, -1.0, -1.0
    L.lib().pcr_icp_plane_default_params(C.byref(p))
    assert (p.max_iter, p.rel_fitness, p.rel_rmse) == (30, 1e-6, 1e-6)
    c = pcp.ICPConvergenceCriteria()
    assert (c.max_iteration, c.relative_fitness, c.relative_rmse) == (30, 1e-6, 1e-6)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_solve_against_numpy(pcp, seed):
    A, b = _system(500, seed)
    st, x, U = _solve(pcp, A, b)
    assert st == pcp._lib.PCR_OK
    ref = np.linalg.solve(A, -b)
    cond = np.linalg.cond(A)
    err, bound = np.linalg.norm(x - ref), 64 * cond * 2.0**-52 * np.linalg.norm(x)
    print(f"seed {seed}: cond(A) = {cond:.3e}  |x - ref| = {err:.3e}  bound = {bound:.3e}")
    assert err <= bound
    # U = [Rz(gamma) Ry(beta) Rx(alpha) | t]
    a, be, g = x[:3]
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(be), 0, np.sin(be)], [0, 1, 0], [-np.sin(be), 0, np.cos(be)]])
    Rz = np.array([[np.cos(g), -np.sin(g), 0], [np.sin(g), np.cos(g), 0], [0, 0, 1]])
    assert np.abs(U[:3, :3] - Rz @ Ry @ Rx).max() <= 1e-15
    assert np.array_equal(U[:3, 3], x[3:])
    assert np.array_equal(U[3], [0.0, 0.0, 0.0, 1.0])


@pytest.mark.parametrize("normal", [(0.0, 0.0, 1.0), (0.6, 0.0, 0.8), (2.0 / 7.0, 3.0 / 7.0, 6.0 / 7.0)])
def test_solve_rank_deficient(pcp, normal):
    """All normals equal: the translation block of A is K n n^T, rank 1."""
    A, b = _system(500, 7, equal_normals=normal)
    assert np.linalg.matrix_rank(A) < 6
    st, x, U = _solve(pcp, A, b)
    assert st == pcp._lib.PCR_E_TOO_FEW_ASSOC
    assert np.array_equal(x, np.zeros(6)) and np.array_equal(U, np.eye(4))


def test_solve_rejects_non_finite_and_null(pcp):
    L = pcp._lib
    A, b = _system(50, 3)
    A[2, 2] = np.nan
    st, _, U = _solve(pcp, A, b)
    assert st == L.PCR_E_TOO_FEW_ASSOC and np.array_equal(U, np.eye(4))
    x = np.zeros(6)
    assert L.lib().pcr_point2plane_solve(None, L.dptr(x), L.dptr(x), L.dptr(x)) == L.PCR_E_INVALID


def test_python_surface_argument_errors(pcp):
    """Checks that need no device: a target without normals and an estimation method that is not built."""
    src = pcp.PointCloud(np.zeros((4, 3)))
    tgt = pcp.PointCloud(np.ones((4, 3)))
    with pytest.raises(RuntimeError, match="normal"):
        pcp.registration_icp(src, tgt, 0.5)

    class TransformationEstimationPointToPoint:
        pass

    tgt.normals = np.tile([0.0, 0.0, 1.0], (4, 1))
    with pytest.raises(NotImplementedError, match="TransformationEstimationPointToPoint"):
        pcp.registration_icp(src, tgt, 0.5, np.eye(4), TransformationEstimationPointToPoint())
