"""pcr_normals and pcr_pca at their paths and edges (tests/neighbourhood_checks.py holds the references and the inputs).

pcr_normals has two producers of every output -- the one-lane 27-cell scan and the redo path (pcr_knn on the left-over rows, one
of its three routes by their number, and a host PCA) -- so every case compares EVERY row: neighbours exactly, in (d2, index) order;
eigenvalues, eigen-residual and direction against a covariance accumulated in np.longdouble, at the tolerances of
tests/pca_checks.py (1e-9 * lambda_1, 1e-9 * lambda_1, 1e-7 where (lambda_2 - lambda_3) / lambda_1 > 1e-4)."""
import functools
import re

import numpy as np
import pytest

from tests import neighbourhood_checks as nc
from tests.pca_checks import check_pca

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def cloud(name):
    if name.startswith("core"):
        return nc.core_and_outliers(int(name[4:]))
    if name == "lattice":
        return nc.lattice(8, 8, 8, 0.25)
    if name == "dups":
        return nc.with_duplicates(nc.core_and_outliers(40), 0.3, seed=5)
    if name == "line":
        return nc.line_cloud(300)
    if name == "plane":
        p = nc.core_and_outliers(0).copy()
        p[:, 2] = 0.25
        return p
    if name == "shifted":
        return nc.core_and_outliers(60) + 1000.0
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name, k):
    return nc.normals_reference(cloud(name), k)


def run_and_check(pcp, name, k, **tol):
    pts = cloud(name)
    got = pcp.estimate_normals(pts, k, return_details=True)
    fig = nc.check_normals_exact(pts, k, got, reference(name, k), **tol)
    print(f"normals {name} k={k}: {fig}")
    return got


@pytest.mark.parametrize("k", range(2, 17))
def test_every_k(pcp, k):
    """Every instantiation of normals_kernel (k = 2..16), 1 620 points of which about 120 go through the redo path."""
    run_and_check(pcp, "core120", k)


@pytest.mark.parametrize("m", sorted(nc.REDO_CLASSES))
@pytest.mark.parametrize("k", [5, 9, 16])
def test_redo_routes(pcp, monkeypatch, capfd, m, k):
    """The number of left-over rows selects the route of pcr_knn (<= 16: one launch of the wave-per-query boxes; 17..255: the
    descent; >= 256: the batched three-stage path, knn_block_kernel<8> or <16> by k).  The library prints the count it handed
    over (PCR_NORMALS_DEBUG, read on every call): it is the count the restated cell formula predicts, and it lies in the class
    the input was built for."""
    name = f"core{m}"
    expect = len(nc.normals_redo_rows(cloud(name), k))
    lo, hi = nc.REDO_CLASSES[m]
    assert lo <= expect <= hi
    monkeypatch.setenv("PCR_NORMALS_DEBUG", "1")
    capfd.readouterr()
    got = run_and_check(pcp, name, k)
    err = capfd.readouterr().err
    assert [int(x) for x in re.findall(r"pcr_normals: redo=(\d+)", err)] == [expect], err
    cell = float(re.search(r"cell=(\S+)", err).group(1))
    assert abs(cell - nc.normals_cell(cloud(name), k)) <= 1e-5 * cell          # (printed with %g)
    monkeypatch.delenv("PCR_NORMALS_DEBUG")
    # the call without details: the same normals, bit for bit
    assert pcp.estimate_normals(cloud(name), k).tobytes() == got[0].tobytes()


@pytest.mark.parametrize("k", [2, 7, 16])
def test_exact_ties_on_a_lattice(pcp, monkeypatch, capfd, k):
    """8 x 8 x 8 lattice, spacing 0.25: every distance ties with others exactly and the cell (< 0.25) sends all 512 rows to the
    redo path (the batched k-NN): ties go to the lower row."""
    monkeypatch.setenv("PCR_NORMALS_DEBUG", "1")
    capfd.readouterr()
    run_and_check(pcp, "lattice", k)
    assert "redo=512" in capfd.readouterr().err


@pytest.mark.parametrize("k", [2, 5, 16])
def test_duplicate_rows(pcp, k):
    """30 % of the rows are exact copies of other rows: distance-0 ties in both producers (about 40 rows are redone)."""
    run_and_check(pcp, "dups", k)


def test_forty_identical_points(pcp):
    """Zero extents: the cell formula yields 0 and the planner takes 1.0.  All forty distances tie: every row's neighbours are
    rows 0..4.  Coordinates that sum exactly give a covariance of exactly zero; others one of the size of the mean's rounding,
    (5 * 2^-53 * |x|)^2 per entry at most."""
    same = np.tile(np.array([[0.5, -1.25, 4.0]]), (40, 1))
    nrm, evs, nbr = pcp.estimate_normals(same, 5, return_details=True)
    assert (nbr == np.arange(5)).all()
    assert not evs.any()
    assert np.isfinite(nrm).all() and np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max() <= 1e-12
    odd = np.tile(np.array([[0.3, -1.2, 4.1]]), (40, 1))
    nrm, evs, nbr = pcp.estimate_normals(odd, 5, return_details=True)
    assert (nbr == np.arange(5)).all()
    assert np.abs(evs).max() <= 3 * 5 / 4 * (5 * 2.0**-53 * 4.1) ** 2
    assert np.isfinite(nrm).all() and np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max() <= 1e-12


@pytest.mark.parametrize("name,k", [("line", 2), ("line", 5), ("line", 16), ("plane", 5), ("plane", 12)])
def test_zero_extents(pcp, monkeypatch, capfd, name, k):
    """A line along x (two zero extents: the planner's emax / 64; 0, 4 and 296 rows redone at k = 2, 5, 16) and a plane of
    constant z (one zero extent: the formula's own cell)."""
    monkeypatch.setenv("PCR_NORMALS_DEBUG", "1")
    capfd.readouterr()
    nrm, evs, nbr = run_and_check(pcp, name, k)
    err = capfd.readouterr().err
    assert f"redo={len(nc.normals_redo_rows(cloud(name), k))}\n" in err, err
    if name == "plane":
        assert np.abs(np.abs(nrm[:, 2]) - 1.0).max() <= 1e-12 and np.abs(evs[:, 2]).max() <= 1e-30
    else:
        assert np.abs(evs[:, 1:]).max() == 0.0 and np.abs(nrm[:, 0]).max() <= 1e-12


@pytest.mark.parametrize("n", [1, 2, 3, 5, 6])
def test_fewer_points_than_k(pcp, n):
    """n <= k = 5: every row holds the n points in (d2, index) order, then -1, and the covariance is of the n points; n = k + 1
    is the first size with a choice to make.  n = 1: include/pcr.h -- zero covariance, eigenvalues 0, normal (0, 0, 1)."""
    pts = np.random.default_rng(n).uniform(-1, 1, (n, 3))
    nrm, evs, nbr = pcp.estimate_normals(pts, 5, return_details=True)
    fig = nc.check_normals_exact(pts, 5, (nrm, evs, nbr))
    assert (nbr[:, min(n, 5):] == -1).all() and (nbr[:, : min(n, 5)] >= 0).all()
    if n == 1:
        assert nbr.tolist() == [[0, -1, -1, -1, -1]] and evs.tolist() == [[0.0, 0.0, 0.0]] and nrm.tolist() == [[0.0, 0.0, 1.0]]
    assert pcp.estimate_normals(pts, 5).tobytes() == nrm.tobytes()
    print(n, fig)


@pytest.mark.parametrize("m,k", [(6, 5), (60, 9), (300, 16)])
def test_purity(pcp, ctx, m, k):
    """One input per redo class: two calls agree bit for bit, and a cloud laid out for another index (records in Morton order,
    id = caller row) gives bit for bit what the fresh upload gives, neighbours included; the cloud is left as it was."""
    pts = cloud(f"core{m}")
    a = pcp.estimate_normals(pts, k, return_details=True)
    b = pcp.estimate_normals(pts, k, return_details=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    dc = pcp.DeviceCloud.upload(pts, ctx)
    index = pcp.TargetIndex(cloud("core120"), kind="grid", ctx=ctx)
    dc.prepare(index)
    c = pcp.estimate_normals(dc, k, return_details=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, c))
    assert pcp.estimate_normals(dc, k).tobytes() == a[0].tobytes()
    assert np.array_equal(dc.download(), pts)
    dc.free()
    index.free()


@pytest.mark.parametrize("k", [5, 16])
def test_cloud_far_from_the_origin(pcp, k):
    """The 60-outlier cloud moved by 1000 m in every coordinate (the reference sees the moved, rounded points too)."""
    run_and_check(pcp, "shifted", k)


# ------------------------------------------------------------------------ PCA
def pca_cloud(n, seed=0):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, 3)) * np.array([3.0, 1.0, 0.2]) + np.array([1.0, -2.0, 0.5])


def pca_with_mean(pcp, ctx, pts):
    L = pcp._lib
    dc = pcp.DeviceCloud.upload(pts, ctx)
    ev, vec, mean = np.empty(3), np.empty((3, 3)), np.empty(3)
    L.check(L.lib().pcr_pca(ctx.handle, dc.handle, L.dptr(ev), L.dptr(vec), L.dptr(mean)), ctx.handle)
    dc.free()
    return ev, vec, mean


@pytest.mark.parametrize("n", [2, 3, 255, 256, 257, 1024, 1025, 262144 + 1])
def test_pca_sizes(pcp, ctx, n):
    """Below, at and above one wave, one block's stride (1024 points per block) and the size at which the grid stops growing (256
    blocks: 262 144 points), against the covariance accumulated in np.longdouble; mean_out against the longdouble mean (a
    thread adds at most 5 values, then 6 + 2 levels of a tree, then 256 partial sums on the host: well under 1e3 roundings of
    2^-53 relative to the largest partial sum, so 1e-12 * max|x| is generous and still 4 digits tighter than a binary32 slip)."""
    pts = pca_cloud(n)
    w_ref, v_ref, mean_ref, _ = nc.pca_reference(pts)
    w, v = pcp.PCA(pts, ctx=ctx)
    check_pca(w, v, w_ref, v_ref)
    w2, v2, mean = pca_with_mean(pcp, ctx, pts)
    assert w2.tobytes() == w.tobytes() and v2.tobytes() == v.tobytes()          # two calls, bit for bit
    assert np.abs(mean - mean_ref).max() <= 1e-12 * np.abs(pts).max()
    wu, vu = pcp.PCA(pts, sort=False, ctx=ctx)
    assert np.array_equal(wu, w[::-1]) and np.array_equal(vu, v[:, ::-1])
    if n == 2:    # rank one: the direction is the difference of the two points
        d = (pts[1] - pts[0]) / np.linalg.norm(pts[1] - pts[0])
        assert abs(abs(v[:, 0] @ d) - 1.0) < 1e-12 and np.abs(w[1:]).max() <= 1e-9 * w[0]
        assert abs(w[0] - 0.5 * np.sum((pts[1] - pts[0]) ** 2)) <= 1e-12 * w[0]


def test_pca_of_one_point(pcp, ctx):
    """np.cov of a single observation is NaN, and so are the eigenvalues (pcr_normals.hip); the mean is the point."""
    w, v, mean = pca_with_mean(pcp, ctx, np.array([[0.3, -1.2, 4.0]]))
    assert np.isnan(w).all()
    assert mean.tolist() == [0.3, -1.2, 4.0]


def test_pca_degenerate_and_shifted(pcp, ctx):
    same = np.tile(np.array([[0.5, -1.25, 4.0]]), (1000, 1))        # (sums exactly: the covariance is exactly zero)
    w, v = pcp.PCA(same, ctx=ctx)
    assert not w.any() and np.allclose(v.T @ v, np.eye(3), atol=1e-12)
    line = nc.line_cloud(300)
    w, v = pcp.PCA(line, ctx=ctx)
    w_ref, v_ref, *_ = nc.pca_reference(line)
    check_pca(w, v, w_ref, v_ref)
    assert w[1] == 0.0 and w[2] == 0.0 and abs(abs(v[0, 0]) - 1.0) <= 1e-12
    plane = pca_cloud(1500, seed=3)
    plane[:, 2] = 0.25
    w, v = pcp.PCA(plane, ctx=ctx)
    w_ref, v_ref, *_ = nc.pca_reference(plane)
    check_pca(w, v, w_ref, v_ref)
    assert w[2] == 0.0 and abs(abs(v[2, 2]) - 1.0) <= 1e-12
    far = pca_cloud(3000, seed=4) + 1e4
    w, v = pcp.PCA(far, ctx=ctx)
    w_ref, v_ref, *_ = nc.pca_reference(far)
    check_pca(w, v, w_ref, v_ref)


def test_pca_prepared_cloud(pcp, ctx):
    """Records in Morton order: another summation order, so within the tolerance, not bit for bit; repeatable; cloud untouched."""
    pts = pca_cloud(5000, seed=5)
    w_ref, v_ref, *_ = nc.pca_reference(pts)
    dc = pcp.DeviceCloud.upload(pts, ctx)
    index = pcp.TargetIndex(pca_cloud(1025, seed=6), kind="grid", ctx=ctx)
    dc.prepare(index)
    w, v = pcp.PCA(dc, ctx=ctx)
    check_pca(w, v, w_ref, v_ref)
    w2, v2 = pcp.PCA(dc, ctx=ctx)
    assert w2.tobytes() == w.tobytes() and v2.tobytes() == v.tobytes()
    assert np.array_equal(dc.download(), pts)
    dc.free()
    index.free()
