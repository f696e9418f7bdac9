"""Every device block has one owner: a call that runs out of device scratch gives everything back and leaves the context usable.

`Context.fail_alloc(n)` makes the n-th next scratch allocation of the context return PCR_E_NOMEM (a counter on the host: nothing is
launched, no device call is made to fail).  Each case below runs its entry point once unarmed, then with the 1st, 2nd, 3rd, ...
allocation refused until the call gets through, and checks after every attempt that the arena holds exactly what it held before
(blocks and bytes), that the failure is PCR_E_NOMEM, that the call that finally succeeds returns the unarmed run's results bit for
bit, and that a fresh registration on the fixture pair still gives the result taken at the start of the module -- an aborted call
must not leave a shared counter word or a pinned landing block dirty.

The cloud is a seeded synthetic object of 513 points (three blocks of 256, the last one partial) whose last 73 rows are replaced by
three isolated points 40 units out (the normals' 3x3x3 block cannot answer them: redo path) and 70 copies of one point (one voxel
above the lane-group threshold: the voxel filter's big-voxel list).  The 300 queries are a slightly moved copy of its first 300 rows
(k-NN with q >= 256 and k <= 16: the three-stage path).  The batch entry points are not swept: their worker threads wait on each
other without a failed state.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_MAX = 128   # loop guard, not a measured number: no listed call takes that many blocks on 513 points


def _rigid(deg, t):
    a = np.array([0.1, 0.2, 1.0]) / np.linalg.norm([0.1, 0.2, 1.0])
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(deg)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = t
    return T


class Env:
    pass


@pytest.fixture(scope="module")
def env(pcp, syn, ctx):
    L = pcp._lib
    e = Env()
    e.pcp, e.L, e.ctx, e.lib = pcp, L, ctx, L.lib()
    P = np.array(syn.object_cloud(513, seed=7), dtype=np.float64)
    P[440:443] = [[40.0, 0.0, 0.0], [0.0, 40.0, 0.0], [0.0, 0.0, 40.0]]
    P[443:] = P[17]
    T = _rigid(1.0, (0.02, -0.01, 0.015))
    Q = np.ascontiguousarray(P[:300] @ T[:3, :3].T + T[:3, 3])
    e.P, e.Q = np.ascontiguousarray(P), Q
    e.P32 = np.ascontiguousarray(P, dtype=np.float32)
    rng = np.random.default_rng(11)
    nrm = rng.normal(size=P.shape)
    e.nrm = np.ascontiguousarray(nrm / np.linalg.norm(nrm, axis=1, keepdims=True))
    e.samples = np.ascontiguousarray(rng.integers(0, 440, size=(8, 3)), dtype=np.int64)
    e.dP = pcp.DeviceCloud.upload(e.P, ctx)
    e.dQ = pcp.DeviceCloud.upload(e.Q, ctx)
    e.grid = pcp.TargetIndex(e.dP, kind="grid", ctx=ctx)
    e.brute = pcp.TargetIndex(e.dP, kind="brute", ctx=ctx)
    e.dQ.prepare(e.grid)   # (the grid searches lay a query cloud out once: done here, so that no case changes a fixture's block)
    e.dP.prepare(e.grid)
    e.prep = []
    for cloud in (e.dQ, e.dP):
        h = C.c_void_p()
        L.check(e.lib.pcr_preprocess(ctx.handle, cloud.handle, 0.1, 0.2, 30, 0.5, 100, C.byref(h)), ctx.handle)
        e.prep.append(h)
    e.icp_ref = _icp(e, e.grid, [])
    yield e
    ctx.fail_alloc(0)
    for h in e.prep:
        e.lib.pcr_prep_free(ctx.handle, h)
    for obj in (e.grid, e.brute, e.dP, e.dQ):
        obj.free()


# ------------------------------------------------------------------ the calls (each frees what it makes, on every path)
def _icp(e, index, keep):
    src = e.pcp.DeviceCloud.upload(e.Q, e.ctx)   # (the passes move the source in place: a fresh one per call)
    try:
        r = e.pcp.icp_device(src, index, np.eye(4), max_iter=2, r_thres=1e-12, t_thres=1e-12, max_d2=5.0)
        moved = src.download()
    finally:
        src.free()
    return [r["T"], r["T_total"], r["iters"], r["status"], r["n_assoc"], r["cost"], r["mean_d2"], np.array(r["R_diff"]), np.array(r["t_diff"]), r["nn_launches"], moved]


def _upload(e, keep, arr):
    c = e.pcp.DeviceCloud.upload(arr, e.ctx)
    try:
        return [c.n, c.download()]
    finally:
        c.free()


def _index_build(e, keep, kind):
    idx = e.pcp.TargetIndex(e.dP, kind=kind, ctx=e.ctx)
    try:
        return [idx.n, idx.cell]
    finally:
        idx.free()


def _nn1(e, keep, index):
    idx, d2 = index.nn1(e.dQ, max_d2=5.0)
    return [idx, d2]


def _moments(e, keep):
    m, o, s = e.grid.moments(e.dQ, max_d2=5.0)
    return [m, o, s]


def _voxel_keys(e, keep):
    h, D = np.zeros(len(e.P)), np.zeros(3)
    keep += [h, D]
    e.L.check(e.lib.pcr_voxel_keys(e.ctx.handle, e.L.dptr(e.P), len(e.P), 0.2, e.L.dptr(h), e.L.dptr(D)), e.ctx.handle)
    return [h, D]


def _voxel_filter(e, keep, mode):
    out, n_out = np.zeros((len(e.P), 3)), C.c_int64()
    keep.append(out)
    e.L.check(e.lib.pcr_voxel_filter(e.ctx.handle, e.L.dptr(e.P), len(e.P), 0.2, mode, 5, e.L.dptr(out), C.byref(n_out)), e.ctx.handle)
    return [n_out.value, out[: n_out.value]]


def _voxel_filter_cloud(e, keep):
    h = C.c_void_p()
    e.L.check(e.lib.pcr_voxel_filter_cloud(e.ctx.handle, e.dP.handle, 0.2, 0, 0, C.byref(h)), e.ctx.handle)
    c = e.pcp.DeviceCloud(e.ctx, h, e.lib.pcr_cloud_size(h))
    try:
        return [c.n, c.download()]
    finally:
        c.free()


def _iss(e, keep, max_kp):
    n = len(e.P)
    lam, counts, kp, nk = np.zeros((n, 3)), np.zeros(n, dtype=np.int32), np.zeros(n + 2, dtype=np.int32), C.c_int()
    keep += [lam, counts, kp]
    e.L.check(e.lib.pcr_iss(e.ctx.handle, e.dP.handle, 0.3, 0.95, 0.95, 0.3, max_kp, e.L.dptr(lam), e.L.iptr(counts), e.L.iptr(kp), C.byref(nk)), e.ctx.handle)
    return [lam, counts, nk.value, kp[: nk.value]]


def _pca(e, keep):
    ev, vec, mean = np.zeros(3), np.zeros(9), np.zeros(3)
    keep += [ev, vec, mean]
    e.L.check(e.lib.pcr_pca(e.ctx.handle, e.dP.handle, e.L.dptr(ev), e.L.dptr(vec), e.L.dptr(mean)), e.ctx.handle)
    return [ev, vec, mean]


def _normals(e, keep):
    n, k = len(e.P), 5
    nrm, ev, nb = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, k), dtype=np.int32)
    keep += [nrm, ev, nb]
    e.L.check(e.lib.pcr_normals(e.ctx.handle, e.dP.handle, k, e.L.dptr(nrm), e.L.dptr(ev), e.L.iptr(nb)), e.ctx.handle)
    return [nrm, ev, nb]


def _knn(e, keep, q, k):
    idx, dist = e.grid.knn(e.Q[:q], k)
    return [idx, dist]


def _radius_counts(e, keep):
    counts = np.zeros(len(e.Q), dtype=np.int64)
    keep.append(counts)
    e.L.check(e.lib.pcr_radius(e.ctx.handle, e.grid.handle, e.L.dptr(e.Q), len(e.Q), 0.3, e.L.lptr(counts), None, None, None), e.ctx.handle)
    return [counts]


def _radius_fill(e, keep):
    counts = e.radius_counts
    offsets = np.zeros(len(e.Q) + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    m = int(offsets[-1])
    idx, dist = np.zeros(m + 1, dtype=np.int32), np.zeros(m + 1)
    keep += [offsets, idx, dist]
    e.L.check(e.lib.pcr_radius(e.ctx.handle, e.grid.handle, e.L.dptr(e.Q), len(e.Q), 0.3, None, e.L.lptr(offsets), e.L.iptr(idx), e.L.dptr(dist)), e.ctx.handle)
    return [idx[:m], dist[:m]]


def _dbscan(e, keep):
    labels, nc = np.zeros(len(e.P), dtype=np.int32), C.c_int32()
    keep.append(labels)
    e.L.check(e.lib.pcr_dbscan(e.ctx.handle, e.dP.handle, 0.15, 4, e.L.iptr(labels), C.byref(nc)), e.ctx.handle)
    return [labels, nc.value]


def _ground(e, keep):
    L, n, n_hyp = e.L, len(e.P), len(e.samples)
    p = L.GroundParams()
    e.lib.pcr_ground_default_params(C.byref(p))
    p.tau, p.ratio, p.n_hyp = 0.05, 0.5, n_hyp
    res, counts = L.GroundResult(), np.zeros(n_hyp, dtype=np.int64)
    rows, mask, h = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8), C.c_void_p()
    keep += [counts, rows, mask]
    L.check(e.lib.pcr_ground_segmentation(e.ctx.handle, e.dP.handle, L.lptr(e.samples), C.byref(p), C.byref(h), L.iptr(rows),
                                          mask.ctypes.data_as(C.POINTER(C.c_uint8)), L.lptr(counts), C.byref(res)), e.ctx.handle, soft=())
    m = int(res.n_outliers)
    c = e.pcp.DeviceCloud(e.ctx, h, m)
    try:
        return [res.best_hyp, res.evaluated, res.n_inliers, m, np.array(res.point[:]), np.array(res.normal[:]), counts, rows[:m], mask, c.download()]
    finally:
        c.free()


def _preprocess(e, keep):
    L, h = e.L, C.c_void_p()
    L.check(e.lib.pcr_preprocess(e.ctx.handle, e.dP.handle, 0.1, 0.2, 30, 0.5, 100, C.byref(h)), e.ctx.handle)
    try:
        n = e.lib.pcr_prep_size(h)
        pts, nrm, f = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 33))
        keep += [pts, nrm, f]
        L.check(e.lib.pcr_prep_download(e.ctx.handle, h, L.dptr(pts), L.dptr(nrm), L.dptr(f)), e.ctx.handle)
        return [n, pts, nrm, f]
    finally:
        e.lib.pcr_prep_free(e.ctx.handle, h)


def _global_registration(e, keep):
    L = e.L
    p, res = L.RansacParams(), L.RansacResult()
    e.lib.pcr_ransac_default_params(C.byref(p))
    p.max_iteration, p.confidence, p.max_distance, p.edge_similarity, p.check_distance, p.seed = 2000, 0.999, 0.15, 0.9, 1, 3
    st = L.check(e.lib.pcr_global_registration(e.ctx.handle, e.prep[0], e.prep[1], C.byref(p), 1, C.byref(res)), e.ctx.handle)
    return [st, np.array(res.T[:]), res.iterations, res.n_valid, res.best_iteration, res.corr_fitness, res.corr_rmse, res.reserved_i]


def _point2plane(e, keep):
    idx = e.pcp.TargetIndex(e.dP, kind="grid", ctx=e.ctx)
    src = None
    try:
        idx.set_normals(e.nrm)
        src = e.pcp.DeviceCloud.upload(e.Q, e.ctx)
        r = e.pcp.icp_point2plane_device(src, idx, np.eye(4), max_correspondence_distance=0.5, max_iteration=3)
        return [r["T"], r["fitness"], r["inlier_rmse"], r["n_corr"], r["iters"], r["status"], np.array(r["fitness_log"]), np.array(r["rmse_log"]), r["nn_launches"]]
    finally:
        if src is not None:
            src.free()
        idx.free()


def _gmm(e, keep):
    L, k = e.L, 2
    p, res = L.GmmParams(), L.GmmResult()
    e.lib.pcr_gmm_default_params(C.byref(p))
    p.n_clusters, p.dim, p.max_iter, p.tol = k, 3, 4, 0.0
    means0 = np.ascontiguousarray(e.P[[3, 200]])
    means, covs, w, hist = np.zeros((k, 3)), np.zeros((k, 3, 3)), np.zeros(k), np.zeros(p.max_iter)
    keep += [means, covs, w, hist]
    L.check(e.lib.pcr_gmm_fit(e.ctx.handle, e.dP.handle, C.byref(p), L.dptr(means0), L.dptr(means), L.dptr(covs), L.dptr(w), L.dptr(hist), C.byref(res)),
            e.ctx.handle, soft=())
    return [means, covs, w, hist[: res.iters], res.iters, res.converged, res.nll, res.passes]


def _kmeans(e, keep):
    L, k = e.L, 3
    p, res = L.KmeansParams(), L.KmeansResult()
    e.lib.pcr_kmeans_default_params(C.byref(p))
    p.n_clusters, p.dim, p.max_iter, p.tol = k, 3, 4, 0.0
    c0 = np.ascontiguousarray(e.P[[3, 200, 441]])
    cen, counts, lab, ih, sh = np.zeros((k, 3)), np.zeros(k, dtype=np.int64), np.zeros(len(e.P), dtype=np.int32), np.zeros(p.max_iter), np.zeros(p.max_iter)
    keep += [cen, counts, lab, ih, sh]
    L.check(e.lib.pcr_kmeans_fit(e.ctx.handle, e.dP.handle, C.byref(p), L.dptr(c0), L.dptr(cen), L.lptr(counts), L.iptr(lab), L.dptr(ih), L.dptr(sh), C.byref(res)),
            e.ctx.handle, soft=())
    return [cen, counts, lab, ih[: res.iters], sh[: res.iters], res.iters, res.converged, res.n_empty, res.inertia, res.shift]


CASES = {
    "cloud_upload_f64": lambda e, keep: _upload(e, keep, e.P),
    "cloud_upload_f32": lambda e, keep: _upload(e, keep, e.P32),
    "cloud_download_f64": lambda e, keep: [e.dP.download()],
    "index_build_grid": lambda e, keep: _index_build(e, keep, "grid"),
    "index_build_brute": lambda e, keep: _index_build(e, keep, "brute"),
    "nn1_grid": lambda e, keep: _nn1(e, keep, e.grid),
    "nn1_brute": lambda e, keep: _nn1(e, keep, e.brute),
    "icp_moments": _moments,
    "icp_grid": lambda e, keep: _icp(e, e.grid, keep),
    "icp_brute": lambda e, keep: _icp(e, e.brute, keep),
    "voxel_keys": _voxel_keys,
    "voxel_filter_mode0": lambda e, keep: _voxel_filter(e, keep, 0),
    "voxel_filter_mode1": lambda e, keep: _voxel_filter(e, keep, 1),
    "voxel_filter_mode2": lambda e, keep: _voxel_filter(e, keep, 2),
    "voxel_filter_cloud": _voxel_filter_cloud,
    "iss_device_suppression": lambda e, keep: _iss(e, keep, 10),
    "iss_host_suppression": lambda e, keep: _iss(e, keep, 1024),   # ISS_NMS_MAX
    "pca": _pca,
    "normals_k5": _normals,
    "knn_q4": lambda e, keep: _knn(e, keep, 4, 8),
    "knn_q300_k8": lambda e, keep: _knn(e, keep, 300, 8),
    "knn_k20": lambda e, keep: _knn(e, keep, 300, 20),
    "radius_counts": _radius_counts,
    "radius_fill": _radius_fill,
    "dbscan": _dbscan,
    "ground_segmentation": _ground,
    "preprocess": _preprocess,
    "global_registration": _global_registration,
    "set_normals_icp_point2plane": _point2plane,
    "gmm_fit": _gmm,
    "kmeans_fit": _kmeans,
}


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def _assert_same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert _same_bits(g, w), f"{what}: output {i} differs"


@pytest.mark.parametrize("name", list(CASES))
def test_refused_allocation_gives_everything_back(env, name):
    e, call = env, CASES[name]
    ctx, L = e.ctx, e.L
    if name == "radius_fill":
        e.radius_counts = _radius_counts(e, [])[0]
    ctx.fail_alloc(0)
    ctx.sync()
    before = ctx.arena_live()
    # 1. unarmed
    keep = []
    want = [np.copy(v) for v in call(e, keep)]
    ctx.sync()
    assert ctx.arena_live() == before, f"{name}: the unarmed call keeps {ctx.arena_live()} against {before} before it"
    # 2. the n-th allocation refused, n = 1, 2, ... until the call gets through
    got, failures = None, 0
    try:
        for n in range(1, N_MAX + 1):
            keep = []
            ctx.fail_alloc(n)
            status = L.PCR_OK
            try:
                got = call(e, keep)
            except L.PcrError as err:
                status = err.status
            ctx.sync()   # (the output arrays in `keep` are still alive)
            assert status in (L.PCR_OK, L.PCR_E_NOMEM), f"{name}: allocation {n} refused -> status {status}"
            assert ctx.arena_live() == before, f"{name}: allocation {n} refused -> arena holds {ctx.arena_live()} against {before} before the call"
            if status == L.PCR_OK:
                break
            failures += 1
        else:
            pytest.fail(f"{name}: no success with any of the first {N_MAX} allocations refused")
    finally:
        ctx.fail_alloc(0)
    # 3. same results, and the context still registers as before
    print(f"{name}: {failures} allocations swept")
    _assert_same(got, want, name)
    _assert_same(_icp(e, e.grid, []), e.icp_ref, f"{name}: registration afterwards")
