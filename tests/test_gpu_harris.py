"""GPU: the PCL-keypoint passes (csrc/pcr_harris.hip: radius normals, Harris-3D response, suppression + selection, corner refinement,
PCL-rule ISS) against the NumPy restatement of include/pcr.h's rules (tests/harris_checks.py).

Tolerances.  The device adds a ball's terms in another order than NumPy: sums of m terms of magnitude <= 1 differ by at most about
m^2 2^-53 per entry (m <= 150 on the object cloud: 2.5e-12), and det / trace^2 amplify that by a small constant -- hence atol 1e-9 on
the response there, and m^2 2^-53 64 per row on the dense cube.  A keypoint decision may differ only where the restatement itself says
it was close (harris_checks: contested / rel_margin)."""
import ctypes as C

import numpy as np
import pytest

from tests import harris_checks as hc

pytestmark = pytest.mark.gpu

RADIUS, THRESHOLD = 0.12, 0.001


@pytest.fixture(scope="module")
def cloud(syn):
    pts = np.ascontiguousarray(syn.object_cloud(2048, seed=2)[:, :3], dtype=np.float64)
    pts.setflags(write=False)
    return pts


@pytest.fixture(scope="module")
def ref(cloud):
    """The restatement end to end (estimated normals), computed once."""
    return hc.harris3d(cloud, RADIUS, THRESHOLD, nms=True)


@pytest.fixture(scope="module")
def gpu(pcp, ctx, cloud):
    """One end-to-end device call on the same cloud, shared by the tests that read it."""
    out, rows, det = pcp.keypointHarris3D(cloud, radius=RADIUS, nms_threshold=THRESHOLD, is_nms=True, return_indices=True, return_details=True, ctx=ctx)
    return {"out": out, "rows": rows, "response": det["response"], "counts": det["counts"]}


def test_response_with_given_normals(pcp, ctx, cloud, ref):
    normals = ref["normals"].copy()
    rng = np.random.default_rng(11)
    normals[rng.random(len(cloud)) < 0.03] = np.nan
    want = hc.response(cloud, RADIUS, normals)
    out, det = pcp.keypointHarris3D(cloud, radius=RADIUS, normals=normals, return_details=True, ctx=ctx)
    got = det["response"]
    assert want["counts"].min() >= 3 and want["counts"].max() <= 150
    err = np.abs(got - want["response"]).max()
    print("given normals: max |response - restated| =", err, "m =", want["counts"].min(), "..", want["counts"].max())
    assert err <= 1e-9
    dead = (want["k"] == 0) | ~np.isfinite(normals).all(axis=1)
    assert dead.sum() >= 30 and (got[dead] == 0.0).all()
    assert np.array_equal(det["counts"], want["counts"])
    assert out.shape == (len(cloud), 4) and out.dtype == np.float32


def test_radius_normals(pcp, ctx, cloud, ref):
    est = ref["estimate"]
    got, counts = pcp.estimate_normals_radius(cloud, RADIUS, ctx=ctx, return_counts=True)
    assert np.array_equal(counts, est["counts"])
    clear = est["gap"] > 1e-3
    assert clear.all()   # every row of this cloud has a determined normal
    dots = np.einsum("ij,ij->i", got, est["normals"])
    print("radius normals: min dot =", dots.min(), "min gap =", est["gap"].min())
    assert (dots[clear] > 1 - 1e-9).all()
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() < 1e-14
    away = pcp.estimate_normals_radius(cloud, RADIUS, viewpoint=(10.0, -20.0, 30.0), ctx=ctx)
    assert (np.einsum("ij,ij->i", away, np.array([10.0, -20.0, 30.0]) - cloud) >= 0).all()
    assert np.array_equal(np.abs(away), np.abs(got))


def test_end_to_end_keypoints(cloud, ref, gpu):
    err = np.abs(gpu["response"] - ref["response"]).max()
    print("end to end: max |response - restated| =", err)
    assert err <= 1e-9   # (the normals agree to ~1e-13 where the eigen-gap is >= 2e-2, as everywhere on this cloud)
    assert np.array_equal(gpu["counts"], ref["counts"])
    cand = ref["candidates"]
    contested = ref["contested"] & cand
    assert cand.sum() == 1578 and len(ref["rows"]) == 34
    assert contested.sum() <= 0.01 * cand.sum()
    differ = np.setxor1d(gpu["rows"], ref["rows"])
    print("end to end: keypoints", len(gpu["rows"]), "restated", len(ref["rows"]), "differing rows", differ, "contested", np.flatnonzero(contested))
    assert ref["contested"][differ].all()
    assert (np.diff(gpu["rows"]) > 0).all()


def test_output_rows_are_positions_and_responses_in_float32(pcp, ctx, cloud, gpu):
    rows = gpu["rows"]
    want = np.concatenate([cloud[rows], gpu["response"][rows, None]], axis=1).astype(np.float32)
    assert gpu["out"].dtype == np.float32 and np.array_equal(gpu["out"], want)
    every, all_rows = pcp.keypointHarris3D(cloud, radius=RADIUS, nms_threshold=THRESHOLD, return_indices=True, ctx=ctx)
    assert every.shape == (2048, 4) and np.array_equal(all_rows, np.arange(2048))
    assert np.array_equal(every, np.concatenate([cloud, gpu["response"][:, None]], axis=1).astype(np.float32))


def test_two_calls_and_a_prepared_cloud_give_the_same_bits(pcp, ctx, cloud, gpu):
    dc = pcp.DeviceCloud.upload(cloud, ctx)
    index = pcp.TargetIndex(cloud + 0.01, kind="grid", ctx=ctx)
    try:
        _, rows1, det1 = pcp.keypointHarris3D(dc, radius=RADIUS, nms_threshold=THRESHOLD, is_nms=True, return_indices=True, return_details=True, ctx=ctx)
        dc.prepare(index)
        assert pcp._lib.lib().pcr_cloud_reordered(dc.handle) == 1
        out2, rows2, det2 = pcp.keypointHarris3D(dc, radius=RADIUS, nms_threshold=THRESHOLD, is_nms=True, return_indices=True, return_details=True, ctx=ctx)
        every = pcp.keypointHarris3D(dc, radius=RADIUS, nms_threshold=THRESHOLD, ctx=ctx)   # every row of a laid-out cloud, by caller row
        assert np.array_equal(every, np.concatenate([cloud, gpu["response"][:, None]], axis=1).astype(np.float32))
    finally:
        index.free()
        dc.free()
    for rows, det in ((rows1, det1), (rows2, det2)):
        assert np.array_equal(rows, gpu["rows"])
        assert np.array_equal(det["response"].view(np.uint64), gpu["response"].view(np.uint64))
        assert np.array_equal(det["counts"], gpu["counts"])
    assert np.array_equal(out2, gpu["out"])   # positions of a device cloud's keypoints are fetched by caller row


@pytest.mark.parametrize("salient,non_max,gamma,n_keypoints", [(0.12, 0.08, 0.8, 91), (0.2, 0.1, 0.975, 52)])
def test_pcl_rule_iss(pcp, ctx, cloud, salient, non_max, gamma, n_keypoints):
    want = hc.iss_pcl(cloud, salient, non_max, gamma, gamma, 5)
    assert len(want["rows"]) == n_keypoints
    out, rows, det = pcp.keypointIss(cloud, salient, non_max, gamma, gamma, 5, return_indices=True, return_details=True, ctx=ctx)
    assert np.array_equal(det["counts"], want["counts"])
    if salient == 0.12:
        assert (want["counts"] < 5).sum() == 217
    # a row's score is zero or not by the ratio tests: where a ratio is within 1e-9 of its gamma either answer stands
    e = want["eigvals"]
    # (and a scatter of rank < 3 -- a ball of one or two rows -- has an e3 that is rounding noise of either sign in any solver)
    with np.errstate(invalid="ignore", divide="ignore"):
        near = (np.abs(e[:, 1] / e[:, 0] - gamma) < 1e-9) | (np.abs(e[:, 2] / e[:, 1] - gamma) < 1e-9)
        flat = ~(e[:, 2] > 1e-9 * e[:, 0])
    both = (det["e3"] > 0) & (want["score"] > 0) & ~flat
    assert np.array_equal((det["e3"] > 0)[~near & ~flat], (want["score"] > 0)[~near & ~flat])
    assert (det["e3"][flat] <= 1e-9 * e[flat, 0]).all()
    rel = np.abs(det["e3"][both] - want["score"][both]) / want["score"][both]
    print("PCL-rule ISS: max relative e3 error =", rel.max(), "keypoints", len(rows), "restated", len(want["rows"]), "near a gamma", near.sum())
    assert rel.max() <= 1e-9
    close = (want["rel_margin"] < 1e-9) | near
    assert close.sum() == 0 or salient != 0.12   # the first configuration has no contested row at all
    differ = np.setxor1d(rows, want["rows"])
    assert close[differ].all()
    if not close.any():
        assert len(rows) == n_keypoints
    assert out.dtype == np.float32 and np.array_equal(out, cloud[rows].astype(np.float32))


@pytest.mark.parametrize("n", [1, 2])
def test_tiny_clouds(pcp, ctx, n):
    pts = np.array([[0.5, 0.25, -1.0], [0.55, 0.25, -1.0]])[:n]
    normals, counts = pcp.estimate_normals_radius(pts, 0.3, ctx=ctx, return_counts=True)
    assert np.isnan(normals).all() and np.array_equal(counts, np.full(n, n))
    kept, rows, det = pcp.keypointHarris3D(pts, radius=0.3, nms_threshold=0.001, is_nms=True, return_indices=True, return_details=True, ctx=ctx)
    assert kept.shape == (0, 4) and len(rows) == 0 and (det["response"] == 0.0).all()
    every = pcp.keypointHarris3D(pts, radius=0.3, nms_threshold=0.001, ctx=ctx)
    assert every.shape == (n, 4) and np.array_equal(every[:, :3], pts.astype(np.float32)) and (every[:, 3] == 0).all()
    assert pcp.keypointIss(pts, 0.3, 0.2, ctx=ctx).shape == (0, 3)


def test_lattice_rows_at_exactly_the_radius(pcp, ctx):
    g = np.arange(5, dtype=np.float64)
    pts = np.stack([m.ravel() for m in np.meshgrid(g, g, g, indexing="ij")], axis=1)
    _, counts = pcp.estimate_normals_radius(pts, 1.0, ctx=ctx, return_counts=True)
    assert np.array_equal(counts, 7 - ((pts == 0) | (pts == 4)).sum(axis=1))
    _, det = pcp.keypointHarris3D(pts, radius=1.0, return_details=True, ctx=ctx)
    assert np.array_equal(det["counts"], counts)


def test_dense_balls(pcp, ctx):
    """3 000 uniform points, r = 0.5: up to ~1 500 rows per ball (many trips of every lane's record loop)."""
    pts = np.random.default_rng(8).uniform(0, 1, (3000, 3))
    normals = np.random.default_rng(9).normal(size=(3000, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    want = hc.response(pts, 0.5, normals)
    _, det = pcp.keypointHarris3D(pts, radius=0.5, normals=normals, return_details=True, ctx=ctx)
    m = want["counts"].astype(np.float64)
    assert m.max() > 1200 and np.array_equal(det["counts"], want["counts"])
    err = np.abs(det["response"] - want["response"])
    print("dense balls: max |response - restated| =", err.max(), "bound at that row =", (m * m * 2.0 ** -53 * 64)[np.argmax(err)], "m max =", m.max())
    assert (err <= m * m * 2.0 ** -53 * 64).all()


def test_extent_beyond_the_grid_is_refused(pcp, ctx):
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 3.0e5, 0.0]])
    for call in (lambda: pcp.keypointHarris3D(pts, radius=1.0, ctx=ctx), lambda: pcp.keypointIss(pts, 1.0, 0.5, ctx=ctx),
                 lambda: pcp.estimate_normals_radius(pts, 1.0, ctx=ctx)):
        with pytest.raises(pcp._lib.PcrError) as e:
            call()
        assert e.value.status == pcp._lib.PCR_E_UNSUPPORTED


def test_small_keypoint_buffer_reports_the_needed_count(pcp, ctx, cloud, gpu):
    L = pcp._lib
    dc = pcp.DeviceCloud.upload(cloud, ctx)
    try:
        p = L.HarrisParams()
        L.lib().pcr_harris_default_params(p)
        p.radius, p.threshold, p.nms = RADIUS, THRESHOLD, 1
        need = len(gpu["rows"])
        kp = np.full(need, -7, dtype=np.int32)
        nk = C.c_int64(-1)
        st = L.lib().pcr_harris3d(ctx.handle, dc.handle, None, p, None, None, L.iptr(kp), need - 1, C.byref(nk), None, None, None)
        assert st == L.PCR_E_UNSUPPORTED and nk.value == need and (kp == -7).all()
        st = L.lib().pcr_harris3d(ctx.handle, dc.handle, None, p, None, None, L.iptr(kp), need, C.byref(nk), None, None, None)
        assert st == L.PCR_OK and nk.value == need and np.array_equal(kp, gpu["rows"])
        nk = C.c_int64(-1)
        st = L.lib().pcr_iss_pcl(ctx.handle, dc.handle, 0.12, 0.08, 0.8, 0.8, 5, None, None, L.iptr(kp), 3, C.byref(nk))
        assert st == L.PCR_E_UNSUPPORTED and nk.value == 91
    finally:
        dc.free()


def test_refine_moves_the_corner_toward_the_true_one(pcp, ctx):
    pts, corner = hc.corner_cloud()
    radius = 0.25
    plain, rows = pcp.keypointHarris3D(pts, radius=radius, nms_threshold=0.001, is_nms=True, return_indices=True, ctx=ctx)
    refined, rows2, det = pcp.keypointHarris3D(pts, radius=radius, nms_threshold=0.001, is_nms=True, is_refine=True, return_indices=True, return_details=True,
                                               ctx=ctx)
    assert np.array_equal(rows, rows2) and len(rows) >= 1
    assert np.array_equal(refined[:, 3], plain[:, 3])   # the intensity stays the unrefined response
    assert (det["rounds"] >= 1).all() and (det["rounds"] <= 5).all()
    k = int(np.argmin(np.linalg.norm(pts[rows] - corner, axis=1)))
    before, after = np.linalg.norm(pts[rows[k]] - corner), np.linalg.norm(refined[k, :3].astype(np.float64) - corner)
    print("refine: corner row", rows[k], "distance before", before, "after", after, "rounds", det["rounds"][k])
    assert after < radius and after <= before
    # the device's refinement against the restated rule, from the device's own normals
    normals = pcp.estimate_normals_radius(pts, radius, ctx=ctx)
    # (at the corner A = sum n n^T has three directions and is well conditioned; along an edge it is nearly singular and the solve
    # amplifies the last bits of the sums, so only the corner is compared: float32 output, coordinates below 2 -> 2.4e-7 of rounding)
    want, want_rounds = hc.refine(pts, normals, radius, pts[rows[k]])
    assert np.abs(refined[k, :3] - want[0]).max() < 1e-6
    assert det["rounds"][k] == want_rounds[0]


def test_ransac_init_with_the_harris_detector(pcp, syn, ctx):
    src, tgt, T_true = syn.perturbed_pair(20000, seed=3)
    R, t, info = pcp.ransac_init(src, tgt, voxel_size=2.0, seed=0, ctx=ctx, detector="harris", return_info=True)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t.ravel()
    assert T.shape == (4, 4) and np.isfinite(T).all()
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-9 and abs(np.linalg.det(R) - 1) < 1e-9
    assert info["detector"] == "harris" and info["n_src_keypoints"] >= 3 and info["n_tgt_keypoints"] >= 3
