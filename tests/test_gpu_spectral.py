"""Spectral clustering on the device (include/pcr.h: pcr_knn_graph, pcr_spectral_fit) against the NumPy restatement of
tests/spectral_checks.py: the graph exactly, the eigenpairs within what their residuals allow (a Ritz value of a symmetric operator
lies within its residual of an eigenvalue; Davis-Kahan for the subspace), the labels against the graph's components and the
restatement's Lloyd, and the edges of the interface.  The restatement of every input is computed once and shared."""
import functools

import numpy as np
import pytest

from tests import spectral_checks as sc
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

TOL = 1e-8
SIZES = (64, 65, 257, 1025, 2049)


@functools.lru_cache(maxsize=None)
def data_of(gen, n):
    return getattr(sc, gen)(n)


@functools.lru_cache(maxsize=None)
def graph_of(gen, n, nnk=7):
    return sc.graph(data_of(gen, n), nnk)


@functools.lru_cache(maxsize=None)
def dense_of(gen, n, normalized):
    return sc.dense(graph_of(gen, n), normalized)


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.abs(b))


# ------------------------------------------------------------------------------------------------------------------ graph
@pytest.mark.parametrize("gen,n,nnk", [("lidar", n, 7) for n in (9,) + SIZES] + [("bridge", 1025, 1), ("bridge", 1025, 15)])
def test_graph_is_exact(pcp, ctx, gen, n, nnk):
    g = graph_of(gen, n, nnk)
    assert g["tie_gap"] > 1e-9 and g["min_dist"] > 0          # nothing that rounding could decide
    indptr, indices, weights = pcp.knn_graph(data_of(gen, n), nnk, ctx=ctx)
    assert indptr.dtype == np.int64 and indices.dtype == np.int32
    assert np.array_equal(indptr, g["indptr"]) and np.array_equal(indices, g["indices"])
    print("weights: largest difference", ulps(weights, g["weights"]).max(), "ulp")
    assert ulps(weights, g["weights"]).max() <= 2
    W = sc.csr({"indptr": indptr, "indices": indices, "weights": weights})
    assert (W != W.T).nnz == 0 and (W.diagonal() == 0).all() and W.nnz == len(indices)
    for r in (0, n // 2, n - 1):
        assert (np.diff(indices[indptr[r]:indptr[r + 1]]) > 0).all()
    assert (np.diff(indptr) >= nnk).all()


# ------------------------------------------------------------------------------------------------------------------ solver
def check_solution(model, lam, U, deg, scale, m, normalized):
    """Residuals, eigenvalues, subspace and the embedding's norm and sign against a dense (or Lanczos) solution."""
    assert model.converged_
    print("residuals", model.residuals_, "iterations", model.n_iter_, "products", model.n_spmm_)
    assert (model.residuals_ <= 2 * TOL).all()
    err = np.abs(model.eigenvalues_ - lam[:m]).max()
    print("eigenvalues: largest difference", err, "bound", scale * 2 * TOL + 1e-12 * scale)
    assert err <= scale * 2 * TOL + 1e-12 * scale
    E = model.embedding_
    assert E.shape == (len(deg), m) and np.isfinite(E).all()
    assert np.abs(np.sqrt((E * E).sum(axis=0)) - 1).max() <= 1e-12
    for j in range(m):
        assert E[np.argmax(np.abs(E[:, j])), j] > 0
    delta = lam[m] - lam[m - 1] if len(lam) > m else np.inf
    if U is not None and delta > 1e-4 * scale:
        Q = np.linalg.qr(E * np.sqrt(deg)[:, None] if normalized else E)[0]
        Ud = U[:, :m]
        sine = np.linalg.norm(Q - Ud @ (Ud.T @ Q), 2)
        bound = 2 * np.sqrt(m) * 2 * TOL * scale / delta + 1e-10
        print("sine of the largest principal angle", sine, "bound", bound, "gap", delta)
        assert sine <= bound


@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("gen", ["lidar", "bridge"])
def test_eigenpairs_against_dense(pcp, ctx, gen, n, normalized):
    d = dense_of(gen, n, normalized)
    g = graph_of(gen, n)
    dc = pcp.DeviceCloud.upload(data_of(gen, n), ctx)
    try:
        for m in (1, 2, 3) + ((8,) if n == 1025 else ()):
            model = pcp.spetral_clustering(m, normalized=normalized).fit(dc, tol=TOL)
            check_solution(model, d["lam"], d["U"], d["deg"], d["scale"], m, normalized)
            assert model.n_edges_ == len(g["indices"]) // 2 and model.max_degree_ == np.diff(g["indptr"]).max()
            assert model.next_eigenvalue_ >= d["lam"][m] - d["scale"] * 1e-9          # a Ritz value of the guard block: never below lambda_{m+1}
            assert (model.n_iter_ == 0) == (n <= 64)
    finally:
        dc.free()


@functools.lru_cache(maxsize=None)
def lanczos_20000():
    """The smallest eigenvalues of the restatement's operator by scipy's eigsh.  A Lanczos process started from one vector finds one
    copy of a repeated eigenvalue, and the three components make 0 a triple one: the operator is block diagonal, so eigsh runs on the
    block of every component and the blocks' eigenvalues are merged."""
    import scipy.sparse.csgraph as csg
    from scipy.sparse.linalg import eigsh
    g = sc.graph(data_of("lidar", 20000), 7)
    B, deg, scale = sc.operator(g, True)
    B = B.tocsr()
    n_comp, comp = csg.connected_components(sc.csr(g), directed=False)
    theta = []
    for c in range(n_comp):
        rows = np.flatnonzero(comp == c)
        theta.extend(eigsh(B[rows][:, rows], k=3, which="LA", tol=1e-12, v0=np.ones(len(rows)))[0])
    return g, deg, np.sort(1.0 - np.array(theta)), n_comp


def test_eigenpairs_20000_against_lanczos(pcp, ctx):
    g, deg, lam, n_comp = lanczos_20000()
    assert g["tie_gap"] > 1e-9 and g["min_dist"] > 0 and n_comp == 3
    model = pcp.spetral_clustering(3).fit(data_of("lidar", 20000), tol=TOL, ctx=ctx)
    check_solution(model, lam, None, deg, 1.0, 3, True)
    print("device ms", model.device_ms_)


# ------------------------------------------------------------------------------------------------------------------ labels
@pytest.mark.parametrize("n", SIZES)
def test_labels_are_the_components(pcp, ctx, n):
    import scipy.sparse.csgraph as csg
    n_comp, comp = csg.connected_components(sc.csr(graph_of("lidar", n)), directed=False)
    assert n_comp == 3
    model = pcp.spetral_clustering(3).fit(data_of("lidar", n), ctx=ctx)
    assert model.labels_.dtype == np.intp and sc.same_partition(model.labels_, comp)
    assert model.seed_rows_[0] == 0 and len(set(comp[model.seed_rows_])) == 3
    assert np.array_equal(model.labels_[model.seed_rows_], [0, 1, 2])          # cluster j is the one seeded by seed j
    assert np.array_equal(model.predict(), model.labels_)


@pytest.mark.parametrize("n", [257, 1025, 2049])
def test_labels_against_the_restated_lloyd(pcp, ctx, n):
    d = dense_of("bridge", n, True)
    E = sc.embedding(d["U"], d["deg"], 2, True)
    km = sc.kmeans_checks.fit(E, E[[0, n - 1]], max_iter=300, tol=1e-4)
    gap = sc.kmeans_checks.predict(E, km["centers"])[2]
    sure = gap > 1e-5
    print("smallest assignment gap", gap.min(), "rows left out", (~sure).sum())
    assert (~sure).sum() <= n // 100
    model = pcp.spetral_clustering(2).fit(data_of("bridge", n), seed_rows=[0, n - 1], ctx=ctx)
    assert np.array_equal(model.seed_rows_, [0, n - 1]) and model.kmeans_converged_
    assert np.array_equal(model.labels_[sure], km["labels"][sure])


@pytest.mark.parametrize("n", [521, 2049])
def test_kmeans_stage_at_eight_clusters(pcp, ctx, n):
    """k = 8 fills every slab slot and every centre row of the K-Means stage.  The restatement runs on the device's own embedding
    from the device's seeds, so the eigensolver's freedom is no part of the comparison; no row is left out."""
    model = pcp.spetral_clustering(8).fit(data_of("chain", n), ctx=ctx)
    E = model.embedding_
    print("solver converged", model.converged_, "iterations", model.n_iter_)
    assert E.shape == (n, 8) and len(set(model.seed_rows_)) == 8
    km = sc.kmeans_checks.fit(E, E[model.seed_rows_], max_iter=300, tol=1e-4)
    print("iterations", km["n_iter"], "smallest assignment gap", km["min_gap"].min())
    assert km["min_gap"].min() > 1e-9          # nothing that rounding could decide
    assert model.kmeans_iter_ == km["n_iter"] and model.kmeans_converged_
    assert np.array_equal(model.labels_, km["labels"])
    assert np.array_equal(np.bincount(model.labels_, minlength=8), km["counts"])
    # sums of n entries of unit-norm columns (|E| <= 1) in another order, then the division
    err = np.abs(model.centers_ - km["centers"]).max()
    rel = abs(model.inertia_ - km["inertia"]) / km["inertia"]
    print("centres: largest difference", err, "bound", 2 * n * 2.0 ** -53, "inertia: relative difference", rel, "bound", n * 2.0 ** -52)
    assert err <= 2 * n * 2.0 ** -53
    assert rel <= n * 2.0 ** -52


@pytest.mark.parametrize("name", ["bridge", "blobs_norm", "blobs_raw"])
def test_golden_partitions(pcp, ctx, name):
    g = load_golden("spectral.npz")
    args = g[name + "_args"]
    data = sc.bridge(int(args[0]), int(args[1])) if name == "bridge" else sc.blobs_even(int(args[0]), int(args[1]))
    model = pcp.spetral_clustering(int(g[name + "_k"]), normalized=bool(g[name + "_normalized"])).fit(data, ctx=ctx)
    assert sc.same_partition(model.labels_, g[name + "_labels"])
    scale = 1.0 if bool(g[name + "_normalized"]) else sc.degrees(sc.graph(data, 7)).max()
    assert np.abs(model.eigenvalues_ - g[name + "_eigenvalues"][:len(model.eigenvalues_)]).max() <= scale * 2 * TOL + 1e-10


# ------------------------------------------------------------------------------------------------------------------ edges
def test_too_small_and_duplicate_rows(pcp, ctx):
    L = pcp._lib
    with pytest.raises(L.PcrError) as e:
        pcp.spetral_clustering(2).fit(data_of("lidar", 9)[:8], ctx=ctx)          # n = nnk + 1: the reference raises IndexError
    assert e.value.status == L.PCR_E_INVALID
    pts = np.array(data_of("lidar", 257))
    pts[200] = pts[31]
    for call in (lambda: pcp.spetral_clustering(3).fit(pts, ctx=ctx), lambda: pcp.knn_graph(pts, ctx=ctx)):
        with pytest.raises(L.PcrError) as e:
            call()
        assert e.value.status == L.PCR_E_SINGULAR and e.value.bad_row == 31
    small = pcp.spetral_clustering(2).fit(data_of("lidar", 9), ctx=ctx)          # n = nnk + 2: the dense path, one component
    d = sc.dense(graph_of("lidar", 9), True)
    assert small.converged_ and np.abs(small.eigenvalues_ - d["lam"][:2]).max() <= 1e-12 and (small.residuals_ <= 1e-12).all()
    assert np.abs(small.embedding_[:, 0] - 1.0 / 3.0).max() <= 1e-12 and abs(np.linalg.norm(small.embedding_[:, 1]) - 1) <= 1e-12
    assert small.n_iter_ == 0 and small.n_edges_ == len(graph_of("lidar", 9)["indices"]) // 2


def test_max_iter_one_returns_the_last_iterate(pcp, ctx):
    model = pcp.spetral_clustering(3).fit(data_of("lidar", 20000), max_iter=1, ctx=ctx)
    assert not model.converged_ and model.n_iter_ == 1 and model.n_spmm_ == 21
    assert np.isfinite(model.embedding_).all() and np.isfinite(model.eigenvalues_).all() and np.isfinite(model.residuals_).all()
    assert (model.residuals_ > 2 * TOL).any() and len(model.labels_) == 20000


def test_prepared_cloud_repeatability_and_side_effects(pcp, ctx):
    pts = data_of("lidar", 2049)
    d = dense_of("lidar", 2049, True)
    np.random.seed(11)
    state = np.random.get_state()
    dc = pcp.DeviceCloud.upload(pts, ctx)
    a = pcp.spetral_clustering(3).fit(dc)
    b = pcp.spetral_clustering(3).fit(dc)
    for key in ("embedding_", "eigenvalues_", "labels_", "residuals_"):
        assert getattr(a, key).tobytes() == getattr(b, key).tobytes(), key
    assert np.array_equal(dc.download(), pts)
    assert np.array_equal(np.random.get_state()[1], state[1]) and np.random.get_state()[2] == state[2]
    index = pcp.TargetIndex(data_of("lidar", 1025), kind="grid", ctx=ctx)
    dc.prepare(index)                      # records in Morton order, id = caller row
    c = pcp.spetral_clustering(3).fit(dc)
    # (inside the triple eigenvalue 0 the basis, and with it the numbering of the clusters, is arbitrary: the partition is not)
    assert sc.same_partition(c.labels_, a.labels_) and c.seed_rows_[0] == 0
    assert c.converged_ and np.abs(c.eigenvalues_ - d["lam"][:3]).max() <= 2 * TOL + 1e-12
    assert np.array_equal(dc.download(), pts)
    # distinct eigenvalues: the same labels
    bpts, bd = data_of("bridge", 2049), dense_of("bridge", 2049, True)
    fresh = pcp.spetral_clustering(2).fit(bpts, ctx=ctx)
    bc = pcp.DeviceCloud.upload(bpts, ctx)
    bc.prepare(index)
    again = pcp.spetral_clustering(2).fit(bc)
    assert np.array_equal(again.labels_, fresh.labels_) and np.array_equal(again.seed_rows_, fresh.seed_rows_)
    assert np.abs(again.eigenvalues_ - bd["lam"][:2]).max() <= 2 * TOL + 1e-12 and np.abs(again.embedding_ - fresh.embedding_).max() <= 1e-4
    assert np.array_equal(bc.download(), bpts)
    for h in (dc, bc, index):
        h.free()


def test_after_ground_segmentation_without_a_download(pcp, ctx):
    import scipy.sparse.csgraph as csg
    rng = np.random.default_rng(3)
    ground = np.column_stack([rng.uniform(-60, 60, 3000), rng.uniform(-60, 60, 3000), -1.7 + rng.normal(0, 0.02, 3000)])
    objects = data_of("lidar", 1025) + np.array([0.0, 0.0, 4.0])
    scene = np.concatenate([ground[:3], objects, ground[3:]])
    dc = pcp.DeviceCloud.upload(scene, ctx)
    seg = pcp.ground_segmentation(dc, samples=np.array([[0, 1, 2]]))
    assert isinstance(seg, pcp.DeviceCloud)
    model = pcp.spetral_clustering(3).fit(seg)
    kept = seg.download()                      # only now, to check
    seg.free()
    dc.free()
    g = sc.graph(kept, 7)
    n_comp, comp = csg.connected_components(sc.csr(g), directed=False)
    assert g["tie_gap"] > 1e-9 and n_comp == 3
    assert model.converged_ and sc.same_partition(model.labels_, comp)


def test_circles_on_which_the_reference_raises(pcp, ctx):
    import scipy.sparse.csgraph as csg
    g = load_golden("spectral.npz")
    assert str(g["circles_reference_raises"]).startswith("ValueError")
    X, y = sc.circles(*[t(v) for t, v in zip((int, float, float, int), g["circles_args"])])
    rg = sc.graph(X, 7)
    n_comp, comp = csg.connected_components(sc.csr(rg), directed=False)
    assert rg["tie_gap"] > 1e-9 and n_comp == 2 and sc.same_partition(comp, y)
    model = pcp.spetral_clustering(2).fit(X, ctx=ctx)
    assert model.converged_ and np.isrealobj(model.embedding_) and np.isfinite(model.embedding_).all()
    assert sc.same_partition(model.labels_, y) and (model.eigenvalues_ <= 2 * TOL).all()
