"""GPU: the PCL-rule FPFH33 at keypoint positions (pcr_fpfh_pcl / pcl_features.fpfh33*) and the k-nearest normals under it
(pcr_normals_knn) against the NumPy restatement of the rules, tests/pcl_fpfh_checks.py.  PARITY UNPINNED: the restatement restates
include/pcr.h, not PCL's binary32 output.

Bounds.  Counts and ``n_spfh`` are integers and equal.  An SPFH value is an integer count times one rounded quotient: the same bits
on both sides whenever the counts agree.  An FPFH value is a sum of K non-negative terms spfh / d^2 -- two roundings each (the
product behind the SPFH, the division) and one addition --, then 11 additions for the block sum and two operations for the scaling,
on both sides: on CLEAN keypoints (no pair that their value depends on within 1e-9 of a bin edge, from the restatement alone; their
share must be >= 0.99)  |got - ref| <= 2 (K + 16) 2^-53 max(got, ref)  elementwise, K the largest ball of the case's keypoints.  On
the other keypoints a pair may cross an edge and nothing else (_check_fpfh's second rule).  NaN rows and zero rows are exact.
The compared cases keep their balls at or below about 400 rows, so that the K^2 pairs under a keypoint leave the clean share alone."""
import ctypes as C

import numpy as np
import pytest

from tests import pcl_fpfh_checks as pf
from tests.test_gpu_fpfh_rows import _states
from tests.test_gpu_global_init_paths import _clean_share, _clusters, _reordered, _unit, _well_share

pytestmark = pytest.mark.gpu

SP_STAGE, FP_STAGE = 128, 256     # pcr_fpfh_pcl.hip: staged positions of the SPFH pass; staged terms of the FPFH pass (consumed past 192)
BALL_CAP = 400                    # what a compared ball may hold
R_SMALL = 0.25


def abi(pcp, ctx, cloud, nrm, kp, radius):
    """pcr_fpfh_pcl itself -> ((m,33) float64, {"counts", "n_spfh"})."""
    L = pcp._lib
    own = None
    if not isinstance(cloud, pcp.DeviceCloud):
        cloud = own = pcp.DeviceCloud.upload(np.ascontiguousarray(cloud, dtype=np.float64), ctx)
    nrm = np.ascontiguousarray(nrm, dtype=np.float64)
    kp = np.ascontiguousarray(kp, dtype=np.float64).reshape(-1, 3)
    assert len(nrm) == cloud.n
    m = len(kp)
    out = np.full((m, 33), -7.0)
    counts = np.full(m, -7, dtype=np.int32)
    n_spfh = C.c_int64(-7)
    try:
        L.check(L.lib().pcr_fpfh_pcl(ctx.handle, cloud.handle, L.dptr(nrm), L.dptr(kp), m, float(radius), L.dptr(out), L.iptr(counts), C.byref(n_spfh)), ctx.handle, soft=())
    finally:
        if own is not None:
            own.free()
    return out, {"counts": counts, "n_spfh": int(n_spfh.value)}


def compare(got, info, ref, values_of=None):
    """The bounds of the module's docstring.  Every condition on the input is asserted on the restatement first.  ``values_of``: the
    keypoints whose values are held to the bound (all of them by default); counts, NaN rows and zero rows are held on every keypoint."""
    values_of = np.ones(len(got), dtype=bool) if values_of is None else values_of
    assert ref["counts"][values_of].max() <= BALL_CAP
    clean = _clean_share(ref["margin"])
    assert np.array_equal(info["counts"], ref["counts"]) and info["n_spfh"] == ref["n_spfh"]
    want = ref["values"]
    empty = ref["counts"] == 0
    assert np.isnan(got[empty]).all() and np.isfinite(got[~empty]).all()
    zero = ~empty & ~np.nan_to_num(want).any(axis=1)
    assert not got[zero].any()
    K = int(ref["counts"][values_of].max())
    sel = clean & ~empty & values_of
    g, r = got[sel], want[sel]
    print("largest |got - ref| on clean keypoints:", np.abs(g - r).max(initial=0.0), "K:", K)
    assert (np.abs(g - r) <= 2 * (K + 16) * 2.0 ** -53 * np.maximum(g, r)).all()
    assert (np.abs(got[~empty] - want[~empty]) > 1e-6).mean() < 0.002


def small_case(syn):
    """The 1 500-point object with random unit normals; 40 rows (unsorted) with three repeated, 10 midpoints between rows (off the
    surface), one point 1e3 away (an empty ball) and one NaN keypoint."""
    pts = syn.object_cloud(1500, seed=3).astype(np.float64)
    rng = np.random.default_rng(11)
    nrm = _unit(rng, len(pts))
    rows40 = rng.choice(len(pts), 40, replace=False)
    assert (np.diff(rows40) < 0).any()
    a, b = rng.choice(len(pts), (2, 10), replace=False)
    kp = np.r_[pts[rows40], pts[rows40[[5, 0, 5]]], (pts[a] + pts[b]) / 2, [pts[0] + [1e3, 0.0, 0.0]], [[np.nan, 0.1, 0.1]]]
    return pts, nrm, kp


@pytest.fixture(scope="module")
def small(pcp, syn, ctx):
    pts, nrm, kp = small_case(syn)
    ref = pf.fpfh33(pts, nrm, kp, R_SMALL)
    got, info = abi(pcp, ctx, pts, nrm, kp, R_SMALL)
    for a in (pts, nrm, kp, got, ref["values"]):
        a.setflags(write=False)
    return dict(pts=pts, nrm=nrm, kp=kp, ref=ref, got=got, info=info)


def test_small_object_against_the_restatement(small):
    ref = small["ref"]
    assert list(ref["counts"][-2:]) == [0, 0] and ref["counts"][:-2].min() >= 2
    assert 40 < ref["n_spfh"] < len(small["pts"])          # a union of balls, not the whole cloud
    compare(small["got"], small["info"], ref)
    assert np.array_equal(small["got"][40:43], small["got"][[5, 0, 5]])


def grid_case(syn):
    """The KITTI-like scan at radius 2.5: the rows on the six bounding faces, the same moved outside the box by 0.5 r and by 2 r, the
    box's eight corners, and 16 rows whose balls stay under the cap."""
    pts = syn.kitti_like_scan(6000, seed=1)[:, :3].astype(np.float64)
    radius = 2.5
    nrm = _unit(np.random.default_rng(8), len(pts))
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    face = np.r_[pts.argmin(axis=0), pts.argmax(axis=0)]
    out = np.r_[-np.eye(3), np.eye(3)]
    corners = np.array([[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)])
    sizes = np.array([len(b) for b in pf.balls(pts, pts, radius)])
    inner = np.random.default_rng(9).choice(np.flatnonzero((sizes > 100) & (sizes <= 300)), 16, replace=False)
    kp = np.r_[pts[face], pts[face] + 0.5 * radius * out, pts[face] + 2.0 * radius * out, corners, pts[inner]]
    return pts, nrm, kp, radius


def test_grid_view_faces_corners_and_outside(pcp, syn, ctx):
    pts, nrm, kp, radius = grid_case(syn)
    ref = pf.fpfh33(pts, nrm, kp, radius)
    assert (ref["counts"][:6] >= 1).all() and not ref["counts"][12:18].any()     # on a face: at least the row; 2 r outside: nothing
    assert ref["counts"][-16:].min() > 100
    got, info = abi(pcp, ctx, pts, nrm, kp, radius)
    # one face row's ball holds 401 rows: past the cap, its counts, block sums and repeatability are compared, its values are not
    under = ref["counts"] <= BALL_CAP
    assert under.sum() == len(kp) - 1
    compare(got, info, ref, values_of=under)
    blocks = got[ref["counts"] > 0].reshape(-1, 3, 11).sum(axis=2)
    assert ((np.abs(blocks - 100.0) <= 1e-10) | (blocks == 0.0)).all()
    again, info2 = abi(pcp, ctx, pts, nrm, kp, radius)
    assert again.tobytes() == got.tobytes() and info2["n_spfh"] == info["n_spfh"]


COUNTS = (1, 2, 3, 63, 64, 65, SP_STAGE - 1, SP_STAGE, SP_STAGE + 1, FP_STAGE - 64 - 1, FP_STAGE - 64, FP_STAGE - 64 + 1, FP_STAGE - 64 + 2, FP_STAGE - 1, FP_STAGE,
          FP_STAGE + 1, FP_STAGE + 2)


def test_ball_sizes_at_the_staging_boundaries(pcp, ctx):
    """Balls of 1, 2, 3 rows, around a wave's 64 lanes, around the SPFH pass's staged positions and around the FPFH pass's staged
    terms (a centre on the surface stages its ball less itself: both count and count - 1 meet every boundary).  One call per centre,
    then all centres at once, the latter also on a re-laid cloud."""
    pts, centre = _clusters(COUNTS, seed=32)
    nrm = _unit(np.random.default_rng(33), len(pts))
    ref = pf.fpfh33(pts, nrm, pts[centre], 1.0)
    assert list(ref["counts"]) == list(COUNTS)
    assert not ref["values"][0].any()                      # the row alone in its ball
    got, info = abi(pcp, ctx, pts, nrm, pts[centre], 1.0)
    compare(got, info, ref)
    for t, c in enumerate(centre):
        one, info1 = abi(pcp, ctx, pts, nrm, pts[[c]], 1.0)
        assert one.tobytes() == got[[t]].tobytes(), COUNTS[t]       # a keypoint's value does not depend on the other keypoints
        assert info1["counts"][0] == COUNTS[t] and info1["n_spfh"] == COUNTS[t]
    moved = _reordered(pcp, pts, ctx)
    relaid, info_r = abi(pcp, ctx, moved, nrm, pts[centre], 1.0)
    moved.free()
    assert relaid.tobytes() == got.tobytes() and info_r["n_spfh"] == info["n_spfh"]


def test_unbounded_balls_succeed(pcp, ctx, small):
    """1 100 copies of one point (without a normal) and 6 rows beside it: every ball holds 1 106 rows, which the hybrid paths refuse
    ("equidistant").  The copies' SPFH is zero -- a keypoint whose ball holds the copies alone gets 33 zeros --, the rows beside them
    pair with each other, and K counts the copies."""
    L = pcp._lib
    rng = np.random.default_rng(41)
    c = np.array([1.0, 2.0, 3.0])
    pts = np.r_[np.tile([c], (1100, 1)), c + np.c_[rng.uniform(0.3, 0.5, 6), rng.uniform(-0.3, 0.3, (6, 2))]]
    nrm = _unit(rng, len(pts))
    nrm[:1100] = np.nan
    kp = np.r_[pts[1100:], pts[:1], [c - [0.75, 0.0, 0.0]]]
    ref = pf.fpfh33(pts, nrm, kp, 1.0)
    assert list(ref["counts"]) == [1106] * 7 + [1100] and ref["n_spfh"] == 1106
    assert not ref["spfh"]["values"][:1100].any() and ref["spfh"]["values"][1100:].any()
    assert _clean_share(ref["margin"]).all()
    before = ctx.arena_live()
    with pytest.raises(L.PcrError) as e:
        pcp.compute_fpfh_at_rows(pts, [1103], _unit(rng, len(pts)), 1.0, 30, ctx=ctx)
    assert e.value.status == L.PCR_E_UNSUPPORTED
    got, info = abi(pcp, ctx, pts, nrm, kp, 1.0)
    assert np.array_equal(info["counts"], ref["counts"]) and info["n_spfh"] == 1106
    assert not got[7].any()                                # the copies' SPFH, at d^2 = 0.5625 each
    assert np.isfinite(got).all() and got[:7].any()
    assert (np.abs(got - ref["values"]) <= 2 * (1106 + 16) * 2.0 ** -53 * np.maximum(got, ref["values"])).all()
    assert ctx.arena_live() == before


def test_rows_without_a_normal_are_skipped_on_both_sides(pcp, ctx, small):
    pts, kp = small["pts"], small["kp"]
    nrm = small["nrm"].copy()
    ball = pf.balls(pts, kp[:1], R_SMALL)[0]
    assert len(ball) > 10
    nrm[ball[[1, 4]]] = np.nan
    nrm[ball[7], 2] = np.inf
    ref = pf.fpfh33(pts, nrm, kp, R_SMALL)
    assert np.abs(np.nan_to_num(ref["values"]) - np.nan_to_num(small["ref"]["values"])).max() > 1e-3      # the case differs from the plain one
    got, info = abi(pcp, ctx, pts, nrm, kp, R_SMALL)
    compare(got, info, ref)


def test_every_cloud_state_gives_the_fresh_upload_s_bytes(pcp, ctx, small):
    pts, nrm, kp = small["pts"], small["nrm"], small["kp"]
    before = ctx.arena_live()
    for name, cloud in _states(pcp, ctx, pts):
        X = cloud.download()
        n = len(X)
        if name == "derived":
            assert 500 < n < len(pts)
        else:
            assert np.array_equal(X, pts), name
        got, info = abi(pcp, ctx, cloud, nrm[:n], kp, R_SMALL)
        fresh, info_fresh = abi(pcp, ctx, X, nrm[:n], kp, R_SMALL)
        cloud.free()
        assert got.tobytes() == fresh.tobytes() and info["n_spfh"] == info_fresh["n_spfh"], name
        assert np.array_equal(info["counts"], info_fresh["counts"]), name
        if name != "derived":
            assert got.tobytes() == small["got"].tobytes(), name
    assert ctx.arena_live() == before


def test_shape_and_order(pcp, ctx, small):
    pts, nrm, kp = small["pts"], small["nrm"], small["kp"]
    n = len(pts)
    a, ia = pcp.fpfh33_with_normal(pts, nrm, kp, R_SMALL, ctx=ctx, return_info=True)
    b, ib = pcp.fpfh33_with_normal(pts, nrm, kp, R_SMALL, ctx=ctx, return_info=True)
    assert a.dtype == np.float32 and a.shape == (len(kp), 33)
    assert a.tobytes() == b.tobytes() and ia["n_spfh"] == ib["n_spfh"] and np.array_equal(ia["counts"], ib["counts"])
    assert a.tobytes() == small["got"].astype(np.float32).tobytes()
    assert (ia["n"], ia["m"]) == (n, len(kp)) and ia["counts"].dtype == np.int32
    perm = np.random.default_rng(10).permutation(len(kp))
    c, ic = pcp.fpfh33_with_normal(pts, nrm, kp[perm], R_SMALL, ctx=ctx, return_info=True)
    assert c.tobytes() == a[perm].tobytes() and ic["n_spfh"] == ia["n_spfh"] and np.array_equal(ic["counts"], ia["counts"][perm])
    finite = kp[:-1]
    want = a[:-1]
    k32 = finite.astype(np.float32)                       # float32 keypoints are other coordinates, the same whatever carries them
    want32 = pcp.fpfh33_with_normal(pts, nrm, k32.astype(np.float64), R_SMALL, ctx=ctx)
    for k in (k32.tolist(), k32, np.repeat(k32, 2, axis=0)[::2], np.c_[k32, np.ones(len(k32), dtype=np.float32)]):
        assert pcp.fpfh33_with_normal(pts, nrm, k, R_SMALL, ctx=ctx).tobytes() == want32.tobytes()
    for k in (finite.tolist(), np.repeat(finite, 2, axis=0)[::2], np.asfortranarray(finite)):
        assert pcp.fpfh33_with_normal(pts, nrm, k, R_SMALL, ctx=ctx).tobytes() == want.tobytes()
    for empty in ([], np.zeros((0, 3))):
        none, info = pcp.fpfh33_with_normal(pts, nrm, empty, R_SMALL, ctx=ctx, return_info=True)
        assert none.shape == (0, 33) and none.dtype == np.float32 and info["n_spfh"] == 0 and info["m"] == 0 and len(info["counts"]) == 0
    one, info = pcp.fpfh33_with_normal(pts, nrm, kp[:1], R_SMALL, ctx=ctx, return_info=True)
    assert one.tobytes() == a[:1].tobytes() and info["n_spfh"] == info["counts"][0] == small["ref"]["counts"][0]
    every, info = pcp.fpfh33_with_normal(pts, nrm, pts, R_SMALL, ctx=ctx, return_info=True)
    assert info["n_spfh"] == n and every.shape == (n, 33) and np.isfinite(every).all()
    cloud = pcp.DeviceCloud.upload(pts, ctx)
    assert pcp.fpfh33_with_normal(cloud, nrm, kp, R_SMALL, ctx=ctx).tobytes() == a.tobytes()
    cloud.free()


def test_errors_leave_nothing_behind(pcp, ctx, small):
    pts, nrm, kp = small["pts"], small["nrm"], small["kp"]
    L = pcp._lib
    before = ctx.arena_live()
    for bad_nrm, bad_kp in ((nrm[:-1], kp), (nrm, np.zeros((4, 2))), (nrm, np.zeros(5))):
        with pytest.raises(ValueError):
            pcp.fpfh33_with_normal(pts, bad_nrm, bad_kp, R_SMALL, ctx=ctx)
    for radius in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(L.PcrError) as e:
            pcp.fpfh33_with_normal(pts, nrm, kp, radius, ctx=ctx)
        assert e.value.status == L.PCR_E_INVALID
    cloud = pcp.DeviceCloud.upload(pts, ctx)
    held = ctx.arena_live()
    out = np.full((2, 33), -7.0)
    k2 = np.ascontiguousarray(kp[:2])
    nr = np.ascontiguousarray(nrm)
    f = L.lib().pcr_fpfh_pcl
    assert f(ctx.handle, cloud.handle, L.dptr(nr), L.dptr(k2), -1, R_SMALL, L.dptr(out), None, None) == L.PCR_E_INVALID
    assert f(ctx.handle, cloud.handle, None, L.dptr(k2), 2, R_SMALL, L.dptr(out), None, None) == L.PCR_E_INVALID
    assert f(ctx.handle, cloud.handle, L.dptr(nr), None, 2, R_SMALL, L.dptr(out), None, None) == L.PCR_E_INVALID
    assert f(ctx.handle, cloud.handle, L.dptr(nr), L.dptr(k2), 2, R_SMALL, None, None, None) == L.PCR_E_INVALID
    assert f(ctx.handle, None, L.dptr(nr), L.dptr(k2), 2, R_SMALL, L.dptr(out), None, None) == L.PCR_E_INVALID
    assert (out == -7.0).all() and ctx.arena_live() == held
    n_spfh = C.c_int64(-7)
    assert f(ctx.handle, cloud.handle, L.dptr(nr), L.dptr(k2), 0, R_SMALL, L.dptr(out), None, C.byref(n_spfh)) == L.PCR_OK       # m = 0: nothing written
    assert (out == -7.0).all() and n_spfh.value == 0
    assert f(ctx.handle, cloud.handle, L.dptr(nr), L.dptr(k2), 2, R_SMALL, L.dptr(out), None, None) == L.PCR_OK                  # the optional outputs may be NULL
    assert out.tobytes() == small["got"][:2].tobytes()
    cloud.free()
    # a cloud whose extent exceeds 2^18 radii
    wide = np.r_[pts, [[3.0e5, 0.0, 0.0]]]
    with pytest.raises(L.PcrError) as e:
        pcp.fpfh33_with_normal(wide, np.r_[nrm, [[0.0, 0.0, 1.0]]], kp, 1.0, ctx=ctx)
    assert e.value.status == L.PCR_E_UNSUPPORTED and b"2^18" in L.lib().pcr_last_error(ctx.handle)
    got, info = abi(pcp, ctx, pts, nrm, kp, R_SMALL)
    assert got.tobytes() == small["got"].tobytes() and info["n_spfh"] == small["info"]["n_spfh"]
    assert ctx.arena_live() == before


def knn_case(syn):
    """The object with five rows far from it: their k nearest rows lie beyond the 3x3x3 block of the normals' grid (the second pass)."""
    pts = syn.object_cloud(1500, seed=3).astype(np.float64)
    far = np.array([[30.0, 1.0, 2.0], [-25.0, 3.0, 1.0], [2.0, 40.0, -3.0], [1.0, -2.0, 35.0], [28.0, 27.0, 3.0]])
    return np.r_[pts, far], (0.4, -0.3, 2.0)


def dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


@pytest.mark.parametrize("k", [3, 10, 16])
def test_knn_normals_against_the_restatement(pcp, syn, ctx, k):
    pts, vp = knn_case(syn)
    ref = pf.knn_normals(pts, k, vp)
    well = _well_share(ref["gap"])
    assert np.abs(dot3(ref["normals"], np.asarray(vp) - pts))[well].min() > 1e-9      # the flip is a sign test: nothing well-conditioned at right angles
    got, curv = pcp.estimate_normals_knn(pts, k, vp, return_curvature=True, ctx=ctx)
    assert got.shape == (len(pts), 3) and curv.shape == (len(pts),)
    assert np.abs(np.linalg.norm(got, axis=1) - 1.0).max() <= 1e-12
    assert (dot3(got[well], ref["normals"][well]) >= 1 - 1e-9).all()
    assert (dot3(got, np.asarray(vp) - pts) >= 0).all()
    assert np.abs(curv - ref["curvature"]).max() <= 1e-9
    assert np.array_equal(pcp.estimate_normals_knn(pts, k, vp, ctx=ctx), got)
    moved = _reordered(pcp, pts, ctx)
    relaid = pcp.estimate_normals_knn(moved, k, vp, ctx=ctx)
    moved.free()
    assert relaid.tobytes() == got.tobytes()
    # the unflipped normals are pcr_normals' own
    plain = pcp.estimate_normals(pts, k=k, ctx=ctx)
    assert np.array_equal(np.abs(plain), np.abs(got))


def test_knn_normals_refuse_what_the_search_cannot_do(pcp, syn, ctx):
    L = pcp._lib
    pts, vp = knn_case(syn)
    before = ctx.arena_live()
    for k in (17, 2, 0, 100):
        with pytest.raises(L.PcrError) as e:
            pcp.estimate_normals_knn(pts, k, vp, ctx=ctx)
        assert e.value.status == L.PCR_E_UNSUPPORTED
        assert b"3 <= k <= 16" in L.lib().pcr_last_error(ctx.handle)
    with pytest.raises(L.PcrError) as e:
        pcp.estimate_normals_knn(pts, 10, (np.nan, 0.0, 0.0), ctx=ctx)
    assert e.value.status == L.PCR_E_INVALID
    two, curv = pcp.estimate_normals_knn(pts[:2], 10, return_curvature=True, ctx=ctx)
    assert np.isnan(two).all() and np.isnan(curv).all()                     # a neighbourhood of fewer than 3 rows
    assert ctx.arena_live() == before


def test_end_to_end(pcp, ctx, small):
    pts, kp = small["pts"], small["kp"]
    vp = (0.4, -0.3, 2.0)
    nrm = pcp.estimate_normals_knn(pts, 10, vp, ctx=ctx)
    a, ia = pcp.fpfh33(pts, kp, 10, R_SMALL, viewpoint=vp, ctx=ctx, return_info=True)
    b, ib = pcp.fpfh33_with_normal(pts, nrm, kp, R_SMALL, ctx=ctx, return_info=True)
    raw, info = abi(pcp, ctx, pts, nrm, kp, R_SMALL)
    assert a.dtype == b.dtype == np.float32
    assert a.tobytes() == b.tobytes() == raw.astype(np.float32).tobytes()
    assert ia["n_spfh"] == ib["n_spfh"] == info["n_spfh"] and np.array_equal(ia["counts"], info["counts"])
    assert np.isnan(a[-2:]).all() and np.isfinite(a[:-2]).all() and a[:-2].any()
    blocks = raw[:-2].reshape(-1, 3, 11).sum(axis=2)
    assert np.abs(blocks - 100.0).max() <= 1e-10
    # the defaults are the wrapper's: k = 10, radius 1.0, the origin as viewpoint
    d = pcp.fpfh33(pts, kp[:4], ctx=ctx)
    e = pcp.fpfh33_with_normal(pts, pcp.estimate_normals_knn(pts, ctx=ctx), kp[:4], ctx=ctx)
    assert d.tobytes() == e.tobytes() and d.shape == (4, 33)
