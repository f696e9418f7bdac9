"""Point-to-plane ICP refinement on the device (refine_registration, Registration/main.py:87-95) against a NumPy restatement of
Open3D's published algorithm, written here ("parity unpinned": Open3D is not importable, the reference holds no fixture).

The restatement evaluates every per-correspondence term with the operations and the order the kernel uses (no fused multiply-add on
either side), so a device sum and a NumPy sum differ only by the order of their additions: each of the 29 sums is held to
4 K 2^-52 sum|term|, twice the forward error bound K 2^-53 sum|term| that either K-term sum obeys in any order.
"""
import functools

import numpy as np
import pytest
from scipy.spatial import cKDTree

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ scenes
def _rot(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def _rigid(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


T_TRUE = _rigid(_rot((0.3, -0.5, 0.8), 2.0), (0.10, -0.07, 0.05))   # the 2-degree offset


def _patches(n, rng):
    """Three separated, mutually orthogonal 4 m square patches, uniform samples, analytic normals."""
    centres = np.array([[0.0, 0.0, 0.0], [10.0, 0.0, 3.0], [0.0, 10.0, 3.0]])
    spans = [(0, 1, 2), (1, 2, 0), (0, 2, 1)]   # (u axis, v axis, normal axis)
    which = np.arange(n) % 3
    uv = rng.uniform(-2.0, 2.0, (n, 2))
    pts, nrm = np.zeros((n, 3)), np.zeros((n, 3))
    for k, (u, v, w) in enumerate(spans):
        sel = which == k
        pts[sel] = centres[k]
        pts[sel, u] += uv[sel, 0]
        pts[sel, v] += uv[sel, 1]
        nrm[sel, w] = 1.0
    return pts, nrm


@functools.lru_cache(maxsize=None)
def scene(n_src, n_tgt, distinct_normals):
    """(source samples on the patches, the same moved by inv(T_TRUE), target points, target normals); read-only arrays."""
    rng = np.random.default_rng(1000 + n_src)
    src, _ = _patches(n_src, rng)
    tgt, nrm = _patches(n_tgt, rng)
    if distinct_normals:   # a wrong row <-> normal mapping cannot cancel
        d = rng.normal(size=nrm.shape)
        nrm = nrm + 0.2 * d / np.linalg.norm(d, axis=1, keepdims=True)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    Ti = np.linalg.inv(T_TRUE)
    moved = src @ Ti[:3, :3].T + Ti[:3, 3]
    for a in (src, moved, tgt, nrm):
        a.setflags(write=False)
    return src, moved, tgt, nrm


# ------------------------------------------------------------- restatement
def _apply(T, P):
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    return np.stack([((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3)], axis=1)


def _d2(S, Q):
    d = S - Q
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


@functools.lru_cache(maxsize=None)
def _tree(key):
    return cKDTree(scene(*key)[2])


def _nearest(S, tgt, tree):
    """exact nearest row (squared distance in the kernel's form, ties to the lower row)"""
    k = 2 if len(tgt) > 1 else 1
    _, i = tree.query(S, k=k)
    i = i.reshape(len(S), k)
    j, d2 = i[:, 0], _d2(S, tgt[i[:, 0]])
    if k == 2:
        d2b = _d2(S, tgt[i[:, 1]])
        swap = (d2b < d2) | ((d2b == d2) & (i[:, 1] < j))
        j, d2 = np.where(swap, i[:, 1], j), np.where(swap, d2b, d2)
    return j, d2


def ref_terms(src, tgt, nrm, tree, T, max_dist):
    """Per-correspondence terms of one pass: (J (K,6), r (K,), d2 (K,))."""
    S = _apply(T, src)
    j, d2 = _nearest(S, tgt, tree)
    keep = d2 < max_dist * max_dist if np.isfinite(max_dist) else np.ones(len(S), dtype=bool)
    S, Q, N, d2 = S[keep], tgt[j[keep]], nrm[j[keep]], d2[keep]
    d = S - Q
    r = (d[:, 0] * N[:, 0] + d[:, 1] * N[:, 1]) + d[:, 2] * N[:, 2]
    sx, sy, sz = S.T
    nx, ny, nz = N.T
    J = np.stack([sy * nz - sz * ny, sz * nx - sx * nz, sx * ny - sy * nx, nx, ny, nz], axis=1)
    return J, r, d2


def ref_icp(src, tgt, nrm, tree, T0, max_dist, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6):
    """Open3D's registration_icp loop with the point-to-plane update, and the header's stated deviation (K < 6 or a singular A stops)."""
    def evaluate(T):
        J, r, d2 = ref_terms(src, tgt, nrm, tree, T, max_dist)
        K = len(r)
        return {"K": K, "fitness": K / len(src) if K else 0.0, "rmse": np.sqrt(d2.sum() / K) if K else 0.0, "J": J, "r": r}

    T = np.array(T0, dtype=np.float64)
    res = evaluate(T)
    log = [res]
    it, status = 0, 0
    for it in range(1, max_iter + 1):
        A, b = res["J"].T @ res["J"], res["J"].T @ res["r"]
        if res["K"] < 6 or np.linalg.matrix_rank(A) < 6:
            it, status = it - 1, 1
            break
        x = np.linalg.solve(A, -b)
        ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
        Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
        Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
        Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
        T = _rigid(Rz @ Ry @ Rx, x[3:]) @ T
        prev, res = res, evaluate(T)
        log.append(res)
        if abs(prev["fitness"] - res["fitness"]) < rel_fitness and abs(prev["rmse"] - res["rmse"]) < rel_rmse:
            break
    return {"T": T, "iters": it, "status": status, "fitness": res["fitness"], "rmse": res["rmse"], "K": res["K"],
            "fitness_log": [e["fitness"] for e in log], "rmse_log": [e["rmse"] for e in log], "K_log": [e["K"] for e in log]}


@functools.lru_cache(maxsize=None)
def ref_icp_cached(n_src, n_tgt, distinct, max_dist):
    _, moved, tgt, nrm = scene(n_src, n_tgt, distinct)
    return ref_icp(moved, tgt, nrm, _tree((n_src, n_tgt, distinct)), np.eye(4), max_dist)


# ---------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def indexed(pcp, ctx):
    """device index with normals per (scene key, kind), built once"""
    made = {}

    def get(key, kind):
        if (key, kind) not in made:
            _, _, tgt, nrm = scene(*key)
            made[(key, kind)] = pcp.TargetIndex(tgt, kind=kind, ctx=ctx).set_normals(nrm)
        return made[(key, kind)]

    yield get
    for ix in made.values():
        ix.free()


def _run(pcp, ctx, source, index, T0=np.eye(4), max_dist=0.5, **kw):
    dev = pcp.DeviceCloud.upload(source, ctx)
    try:
        return pcp.icp_point2plane_device(dev, index, T0, max_correspondence_distance=max_dist, **kw)
    finally:
        dev.free()


# ------------------------------------------------------------------- tests
MOMENT_CASES = [(1, 300, "grid"), (63, 300, "grid"), (257, 300, "grid"), (4099, 5000, "grid"), (300001, 50000, "grid"),
                (1, 300, "brute"), (63, 300, "brute"), (257, 300, "brute"), (4099, 5000, "brute")]


@pytest.mark.parametrize("max_dist", [0.5, np.inf])
@pytest.mark.parametrize("n_src,n_tgt,kind", MOMENT_CASES)
def test_moments_against_numpy(pcp, ctx, indexed, n_src, n_tgt, kind, max_dist):
    """1. one pass: K equal, each of the 28 sums within 4 K 2^-52 sum|term| (300 001 sources: the capped grid strides twice)."""
    key = (n_src, n_tgt, True)
    src, _, tgt, nrm = scene(*key)
    J, r, d2 = ref_terms(src, tgt, nrm, _tree(key), T_TRUE, max_dist)
    A, b, K, sd2 = indexed(key, kind).point2plane_moments(src, T_TRUE, max_dist)
    assert K == len(r)
    if np.isfinite(max_dist) and n_src == 257:
        assert K < n_src   # the gate is exercised
    u = 4.0 * K * 2.0**-52
    worst = 0.0
    for i in range(6):
        for j in range(6):
            terms = J[:, i] * J[:, j]
            err, tol = abs(A[i, j] - terms.sum()), u * np.abs(terms).sum()
            worst = max(worst, err / tol if tol else err)
            assert err <= tol, ("A", i, j, err, tol)
        terms = J[:, i] * r
        err, tol = abs(b[i] - terms.sum()), u * np.abs(terms).sum()
        worst = max(worst, err / tol if tol else err)
        assert err <= tol, ("b", i, err, tol)
    err, tol = abs(sd2 - d2.sum()), u * d2.sum()
    assert err <= tol, ("sum d2", err, tol)
    print(f"n={n_src} {kind} gate={max_dist}: K={K}, worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("n_src,n_tgt", [(4099, 5000), (257, 300)])
@pytest.mark.parametrize("kind", ["grid", "brute"])
def test_loop_parity(pcp, ctx, indexed, kind, n_src, n_tgt):
    """2. the whole loop against the restatement: distinct normals, gate 0.5 (at 257 / 300 the gate's set changes between iterations)."""
    key = (n_src, n_tgt, True)
    ref = ref_icp_cached(*key, 0.5)
    res = _run(pcp, ctx, scene(*key)[1], indexed(key, kind))
    print(f"{kind}: iters {res['iters']} (ref {ref['iters']}), |T - T_ref| = {np.abs(res['T'] - ref['T']).max():.3e}, "
          f"rmse log diff = {np.abs(np.array(res['rmse_log']) - np.array(ref['rmse_log'])).max():.3e}")
    if n_src == 257:
        assert ref["K_log"][0] < ref["K_log"][-1] < n_src   # the gate is exercised
    assert res["status"] == 0 and res["iters"] == ref["iters"]
    assert len(res["fitness_log"]) == len(ref["fitness_log"]) == res["iters"] + 1
    assert [int(round(f * n_src)) for f in res["fitness_log"]] == ref["K_log"] and res["n_corr"] == ref["K"]
    assert res["fitness_log"] == ref["fitness_log"] and res["fitness"] == ref["fitness"]
    assert np.abs(res["T"] - ref["T"]).max() <= 1e-9
    assert np.abs(np.array(res["rmse_log"]) - np.array(ref["rmse_log"])).max() <= 1e-9
    assert res["inlier_rmse"] == res["rmse_log"][-1]


@pytest.mark.parametrize("n_src,n_tgt", [(4099, 5000), (33001, 40000)])
@pytest.mark.parametrize("max_dist", [0.5, 1.0])
def test_recovers_truth(pcp, ctx, indexed, n_src, n_tgt, max_dist):
    """3. exact planes: the known motion comes back (the restatement itself is within 4e-15 of it)."""
    key = (n_src, n_tgt, False)
    res = _run(pcp, ctx, scene(*key)[1], indexed(key, "grid"), max_dist=max_dist)
    print(f"{n_src}/{n_tgt} gate {max_dist}: iters {res['iters']}, |T - truth| = {np.abs(res['T'] - T_TRUE).max():.3e}")
    assert np.abs(res["T"] - T_TRUE).max() <= 1e-9
    assert res["fitness"] == 1.0 and res["n_corr"] == n_src
    assert res["iters"] <= 5 and res["status"] == 0


def test_restatement_recovers_truth():
    ref = ref_icp_cached(4099, 5000, False, 0.5)
    assert np.abs(ref["T"] - T_TRUE).max() <= 1e-13 and ref["fitness"] == 1.0 and ref["iters"] <= 5


@pytest.mark.parametrize("kind", ["grid", "brute"])
def test_deterministic_and_pure(pcp, ctx, indexed, kind):
    """4. same call twice: identical bits; the source cloud is not modified."""
    key = (4099, 5000, True)
    moved = scene(*key)[1]
    dev = pcp.DeviceCloud.upload(moved, ctx)
    try:
        a = pcp.icp_point2plane_device(dev, indexed(key, kind), np.eye(4), max_correspondence_distance=0.5)
        b = pcp.icp_point2plane_device(dev, indexed(key, kind), np.eye(4), max_correspondence_distance=0.5)
        after = dev.download()
    finally:
        dev.free()
    assert a["T"].tobytes() == b["T"].tobytes()
    assert np.array(a["rmse_log"]).tobytes() == np.array(b["rmse_log"]).tobytes() and a["fitness_log"] == b["fitness_log"]
    assert (a["iters"], a["n_corr"], a["inlier_rmse"]) == (b["iters"], b["n_corr"], b["inlier_rmse"])
    assert after.tobytes() == moved.tobytes()
    m1 = indexed(key, kind).point2plane_moments(moved, T_TRUE, 0.5)
    m2 = indexed(key, kind).point2plane_moments(moved, T_TRUE, 0.5)
    assert m1[0].tobytes() == m2[0].tobytes() and m1[1].tobytes() == m2[1].tobytes() and m1[2:] == m2[2:]


@pytest.mark.parametrize("kind", ["grid", "brute"])
def test_edges(pcp, ctx, indexed, kind):
    """5. missing normals, nothing inside the gate, max_iter 0 and 257."""
    L = pcp._lib
    key = (257, 300, True)
    _, moved, tgt, nrm = scene(*key)
    index = indexed(key, kind)
    bare = pcp.TargetIndex(tgt, kind=kind, ctx=ctx)
    try:
        assert not bare.has_normals and index.has_normals
        with pytest.raises(RuntimeError) as e:
            _run(pcp, ctx, moved, bare)
        assert e.value.status == L.PCR_E_INVALID
        bad = np.array(nrm)
        bad[17, 1] = np.inf
        with pytest.raises(L.PcrError) as e:
            bare.set_normals(bad)
        assert e.value.status == L.PCR_E_INVALID and not bare.has_normals
        zero = np.array(nrm)
        zero[5] = 0.0
        bare.set_normals(zero)   # zero-length normals are accepted
        assert bare.has_normals
    finally:
        bare.free()
    T0 = _rigid(_rot((1, 2, 3), 5.0), (0.01, 0.02, 0.03))
    far = _run(pcp, ctx, moved + np.array([0.0, 0.0, 100.0]), index, T0)
    assert far["status"] == L.PCR_E_TOO_FEW_ASSOC and far["iters"] == 0
    assert np.array_equal(far["T"], T0) and far["fitness"] == 0.0 and far["inlier_rmse"] == 0.0 and far["n_corr"] == 0
    none = _run(pcp, ctx, moved, index, T0, max_iteration=0)
    J, r, d2 = ref_terms(moved, tgt, nrm, _tree(key), T0, 0.5)
    assert np.array_equal(none["T"], T0) and none["iters"] == 0 and none["status"] == 0
    assert none["n_corr"] == len(r) and none["fitness"] == len(r) / 257
    rmse = np.sqrt(d2.sum() / len(r))   # a K-term sum in another order: relative 4 K 2^-52 at most, half of that behind the root
    assert abs(none["inlier_rmse"] - rmse) <= 2 * len(r) * 2.0**-52 * rmse
    with pytest.raises(L.PcrError) as e:
        _run(pcp, ctx, moved, index, max_iteration=257)
    assert e.value.status == L.PCR_E_TOO_MANY_ITERS


def test_python_surface(pcp, ctx):
    """6. refine_registration from a RegistrationResult holding the 2-degree offset; normals given, and estimated when absent."""
    src, _, tgt, nrm = scene(4099, 5000, False)
    ransac = pcp.RegistrationResult(T_TRUE)
    voxel_size = 1.25   # threshold 0.5, normal radius 2.5
    target = pcp.PointCloud(tgt)
    source = pcp.PointCloud(src)
    est = pcp.refine_registration(source, target, None, None, voxel_size, ransac, ctx=ctx)
    assert not hasattr(target, "normals") and np.array_equal(source.points, src)
    target.normals = nrm
    given = pcp.refine_registration(source, target, None, None, voxel_size, ransac, ctx=ctx)
    for res in (est, given):
        assert isinstance(res, pcp.RegistrationResult)
        print(f"|T - I| = {np.abs(res.transformation - np.eye(4)).max():.3e}, fitness {res.fitness}, iterations {res.info['iters']}")
        assert np.abs(res.transformation - np.eye(4)).max() <= 1e-9
        assert res.fitness == 1.0 and res.info["status"] == 0 and res.info["iters"] <= 5
    index = pcp.TargetIndex(tgt, ctx=ctx).set_normals(nrm)
    try:
        via_index = pcp.registration_icp(source, index, 0.5, T_TRUE, pcp.TransformationEstimationPointToPlane(),
                                         pcp.ICPConvergenceCriteria(max_iteration=30))
    finally:
        index.free()
    assert via_index.transformation.tobytes() == given.transformation.tobytes()
