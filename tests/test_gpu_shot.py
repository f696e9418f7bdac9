"""GPU: SHOT352 at keypoint positions (pcr_shot_lrf, pcr_shot352 / pcl_features.shot352*) against the NumPy restatement of the rules,
tests/shot_checks.py.  PARITY UNPINNED: the restatement restates include/pcr.h, not PCL's binary32 output.

Frames.  Counts are integers and equal.  The moment sums run in another order on the device and the eigenvectors come from another
solver, so a frame is compared where it is well conditioned -- eigenvalue gaps > 1e-3 of e2 and no neighbour within 1e-9 of either
sign plane, from the restatement alone; the share of such keypoints must be >= 0.9 --: every row within 1 - 1e-9 of the restatement's
with the same sign (what tests/test_gpu_harris.py holds radius normals to at that gap), unit rows to 1e-14, a right-handed frame.

Histogram, from the device's OWN frames fed to the restatement.  Every hard decision (ball, skip, volume, step, branch) is then taken on
the same bits by the same binary64 operations, and every contribution is the same number before it is quantised, but for three of a
neighbour's at most six: the elevation share, the azimuth share and W hold acos / atan2, which differ between the two libms.  OpenCL's
bounds for binary64 (acos 4 ulp, atan2 6 ulp; a correctly rounded host: 1) put theta within 5 ulp(pi) = 5 2^-51 and the angle within
7 2^-51, so u moves by <= 5 2^-51 / (pi/2) < 7 2^-52, a by <= 7 2^-51 / (pi/4) < 18 2^-52 and W by their sum: < 6e-15 each, or
2.4e-5 of a unit of 2^-32 once scaled.  A branch on theta or on a that goes the other way does so where its two sides agree (u or a
is 0 there), so it moves no more.  rint then moves a contribution by at most ONE unit, and with `used` neighbours not skipped
    sum_b |dh_b| <= 3 used 2^-32,   hence  |dh_b| <= 3 used 2^-32  and  | |h + dh| - |h| | <= 3 used 2^-32.
out_b = h_b / |h|:  |d out_b| <= |dh_b| / |h| + (h_b / |h|) d|h| / |h| <= 6 used 2^-32 / |h|.  The norm's 352 squares and 351 additions
in another order, its root and the division add a relative (352 + 4) 2^-53 on each side, on out_b <= 1:
    |got_b - ref_b| <= 6 used 2^-32 / |h| + 720 2^-53,      |h| from the restatement's integer histogram.
(Every neighbour that is not skipped adds >= 2 in all, so |h| >= 2 used / sqrt(352) and the first term is <= 57 2^-32 whatever the
ball.)  NaN rows are exactly the NaN rows.  Measured on an MI355X: DESIGN.md section 3.6.0.2."""
import numpy as np
import pytest

from tests import pcl_fpfh_checks as pf
from tests import shot_checks as sc
from tests.test_gpu_fpfh_rows import _states
from tests.test_gpu_global_init_paths import _clusters, _reordered, _unit
from tests.test_gpu_pcl_fpfh import grid_case, small_case
from tests.test_shot_host import _mirrored

pytestmark = pytest.mark.gpu

SHOT_STAGE = 128                  # pcr_shot.hip: staged in-ball entries of the tie walk and of the histogram walk, consumed 64 at a time
R_SMALL = 0.25


def abi(pcp, ctx, cloud, nrm, kp, radius, frames_in=None):
    """pcr_shot352 itself -> ((m,352) float64, frames (m,3,3), counts (m,) int32)."""
    L = pcp._lib
    own = None
    if not isinstance(cloud, pcp.DeviceCloud):
        cloud = own = pcp.DeviceCloud.upload(np.ascontiguousarray(cloud, dtype=np.float64), ctx)
    nrm = np.ascontiguousarray(nrm, dtype=np.float64)
    kp = np.ascontiguousarray(kp, dtype=np.float64).reshape(-1, 3)
    assert len(nrm) == cloud.n
    m = len(kp)
    fin = None
    if frames_in is not None:
        fin = np.ascontiguousarray(frames_in, dtype=np.float64).reshape(m, 9)
    out = np.full((m, 352), -7.0)
    frames = np.full((m, 9), -7.0)
    counts = np.full(m, -7, dtype=np.int32)
    try:
        L.check(L.lib().pcr_shot352(ctx.handle, cloud.handle, L.dptr(nrm), L.dptr(kp), m, float(radius), L.dptr(fin) if fin is not None else None, L.dptr(out),
                                    L.dptr(frames), L.iptr(counts)), ctx.handle, soft=())
    finally:
        if own is not None:
            own.free()
    return out, frames.reshape(m, 3, 3), counts


def abi_lrf(pcp, ctx, cloud, kp, radius):
    """pcr_shot_lrf itself -> (frames (m,3,3), counts (m,) int32)."""
    L = pcp._lib
    own = None
    if not isinstance(cloud, pcp.DeviceCloud):
        cloud = own = pcp.DeviceCloud.upload(np.ascontiguousarray(cloud, dtype=np.float64), ctx)
    kp = np.ascontiguousarray(kp, dtype=np.float64).reshape(-1, 3)
    m = len(kp)
    frames = np.full((m, 9), -7.0)
    counts = np.full(m, -7, dtype=np.int32)
    try:
        L.check(L.lib().pcr_shot_lrf(ctx.handle, cloud.handle, L.dptr(kp), m, float(radius), L.dptr(frames), L.iptr(counts)), ctx.handle, soft=())
    finally:
        if own is not None:
            own.free()
    return frames.reshape(m, 3, 3), counts


def check_frames(frames, counts, ref, min_share=0.9):
    """The frame rules of the module's docstring; ``ref`` = shot_checks.lrf of the same case."""
    assert np.array_equal(counts, ref["counts"])
    none = np.isnan(ref["frames"]).all(axis=(1, 2))
    assert np.array_equal(none, ref["counts"] < 5)
    assert np.isnan(frames[none]).all() and np.isfinite(frames[~none]).all()
    good = ~none & (ref["gap"] > 1e-3) & (ref["sign_margin"] > 1e-9)
    share = good[~none].mean()
    print("well-conditioned share:", share, "ties among them:", int(ref["tie"][good].any(axis=1).sum()))
    assert share >= min_share
    dots = np.einsum("kij,kij->ki", frames[good], ref["frames"][good])
    print("smallest row dot:", dots.min(initial=1.0))
    assert (dots > 1 - 1e-9).all()
    F = frames[~none]
    assert np.abs(np.linalg.norm(F, axis=2) - 1.0).max() <= 1e-14
    assert (np.linalg.det(F) > 0).all()
    return good


def check_values(got, frames, counts, pts, nrm, kp, radius):
    """The histogram bound of the module's docstring, the device's own frames fed to the restatement.  -> the restatement's dict."""
    ref = sc.shot352(pts, nrm, kp, radius, frames=frames)
    assert np.array_equal(counts, ref["counts"])
    nan = np.isnan(ref["values"]).any(axis=1)
    assert np.isnan(got[nan]).all() and np.isfinite(got[~nan]).all()
    norm = np.sqrt(((ref["hist"][~nan] * 2.0 ** -32) ** 2).sum(axis=1))
    bound = 6 * ref["used"][~nan] * 2.0 ** -32 / norm + 720 * 2.0 ** -53
    assert (bound <= 57 * 2.0 ** -32 + 720 * 2.0 ** -53).all()
    dev = np.abs(got[~nan] - ref["values"][~nan])
    equal = (got[~nan] == ref["values"][~nan]).all(axis=1)
    print("largest |got - ref|:", dev.max(initial=0.0), "in units of 2^-32:", dev.max(initial=0.0) * 2.0 ** 32, "smallest bound:", bound.min(initial=np.inf),
          "byte-equal rows:", int(equal.sum()), "of", len(equal))
    assert (dev <= bound[:, None]).all()
    return ref


@pytest.fixture(scope="module")
def small(pcp, syn, ctx):
    pts, nrm, kp = small_case(syn)
    got, frames, counts = abi(pcp, ctx, pts, nrm, kp, R_SMALL)
    ref_lrf = sc.lrf(pts, kp, R_SMALL)
    for a in (pts, nrm, kp, got, frames, counts):
        a.setflags(write=False)
    return dict(pts=pts, nrm=nrm, kp=kp, got=got, frames=frames, counts=counts, ref_lrf=ref_lrf)


def test_small_object_frames_against_the_restatement(pcp, ctx, small):
    ref = small["ref_lrf"]
    assert list(ref["counts"][-2:]) == [0, 0] and ref["counts"][:-2].min() >= 5
    good = check_frames(small["frames"], small["counts"], ref)
    assert good[:-2].all()                                  # (checked on the host: every gap of this case is >= 0.02 and none ties)
    lrf, counts = abi_lrf(pcp, ctx, small["pts"], small["kp"], R_SMALL)
    assert lrf.tobytes() == small["frames"].tobytes() and np.array_equal(counts, small["counts"])
    assert np.array_equal(small["frames"][40:43], small["frames"][[5, 0, 5]])


def test_small_object_histogram_against_the_restatement(small):
    ref = check_values(small["got"], small["frames"], small["counts"], small["pts"], small["nrm"], small["kp"], R_SMALL)
    assert np.isnan(small["got"][-2:]).all() and (ref["used"][:-2] >= 5).all()
    fin = small["got"][:-2]
    assert np.abs(np.linalg.norm(fin, axis=1) - 1.0).max() <= 720 * 2.0 ** -53 and (fin >= 0).all()
    assert np.array_equal(small["got"][40:43], small["got"][[5, 0, 5]])            # repeated keypoints give equal rows


def test_grid_view_faces_corners_and_outside(pcp, syn, ctx):
    pts, nrm, kp, radius = grid_case(syn)
    ref = sc.lrf(pts, kp, radius)
    assert not ref["counts"][12:18].any() and ref["counts"][-16:].min() > 100
    got, frames, counts = abi(pcp, ctx, pts, nrm, kp, radius)
    good = check_frames(frames, counts, ref, min_share=0.0)                        # faces and corners: thin balls, whatever their gaps are
    assert good[-16:].all()                                                        # (the 16 inner rows: every gap >= 0.039)
    check_values(got, frames, counts, pts, nrm, kp, radius)
    again, frames2, _ = abi(pcp, ctx, pts, nrm, kp, radius)
    assert again.tobytes() == got.tobytes() and frames2.tobytes() == frames.tobytes()


def test_given_frames_replace_the_frame_stage(pcp, ctx, small):
    pts, nrm, kp = small["pts"], small["nrm"], small["kp"]
    # the frames of an earlier call: its bytes
    got, frames, counts = abi(pcp, ctx, pts, nrm, kp, R_SMALL, frames_in=small["frames"])
    assert got.tobytes() == small["got"].tobytes() and frames.tobytes() == small["frames"].tobytes() and np.array_equal(counts, small["counts"])
    # the restatement's frames: the bound against the restatement end to end
    ref = sc.shot352(pts, nrm, kp, R_SMALL)
    got, frames, counts = abi(pcp, ctx, pts, nrm, kp, R_SMALL, frames_in=ref["frames"])
    assert frames.tobytes() == ref["frames"].tobytes()
    check_values(got, ref["frames"], counts, pts, nrm, kp, R_SMALL)
    # a row with an entry that is not finite: NaN, the other rows as they were; identity frames where the rule gives none
    mixed = small["frames"].copy()
    mixed[3, 1, 2] = np.inf
    mixed[-2:] = np.eye(3)
    got, frames, counts = abi(pcp, ctx, pts, nrm, kp, R_SMALL, frames_in=mixed)
    assert np.isnan(got[3]).all() and got[:3].tobytes() == small["got"][:3].tobytes() and got[4:-2].tobytes() == small["got"][4:-2].tobytes()
    assert np.isnan(got[-2:]).all() and list(counts[-2:]) == [0, 0]                # an empty ball: a zero norm


COUNTS = (1, 4, 5, 6, 63, 64, 65, 127, SHOT_STAGE, SHOT_STAGE + 1, 191, 192, 193)


def test_ball_sizes_at_the_staging_boundaries(pcp, ctx):
    """Balls of 1 .. 6 rows (no frame below 5), around a wave's 64 lanes and around the staged entries (a centre on the surface stages
    its ball, and skips itself in the histogram).  One call per centre, then all centres at once, the latter also on a re-laid cloud."""
    pts, centre = _clusters(COUNTS, seed=32)
    nrm = _unit(np.random.default_rng(33), len(pts))
    kp = pts[centre]
    before = ctx.arena_live()
    got, frames, counts = abi(pcp, ctx, pts, nrm, kp, 1.0)
    assert list(counts) == list(COUNTS)
    check_frames(frames, counts, sc.lrf(pts, kp, 1.0), min_share=0.0)
    check_values(got, frames, counts, pts, nrm, kp, 1.0)
    assert np.isnan(got[:2]).all() and np.isfinite(got[2:]).all()
    for t, c in enumerate(centre):
        one, f1, c1 = abi(pcp, ctx, pts, nrm, pts[[c]], 1.0)
        assert one.tobytes() == got[[t]].tobytes() and f1.tobytes() == frames[[t]].tobytes(), COUNTS[t]    # a keypoint does not depend on the others
        assert c1[0] == COUNTS[t]
    moved = _reordered(pcp, pts, ctx)
    relaid, f_r, c_r = abi(pcp, ctx, moved, nrm, kp, 1.0)
    lrf_r, _ = abi_lrf(pcp, ctx, moved, kp, 1.0)
    moved.free()
    assert relaid.tobytes() == got.tobytes() and f_r.tobytes() == frames.tobytes() and lrf_r.tobytes() == frames.tobytes() and np.array_equal(c_r, counts)
    assert ctx.arena_live() == before


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
        got, frames, counts = abi(pcp, ctx, cloud, nrm[:n], kp, R_SMALL)
        fresh, frames_fresh, counts_fresh = abi(pcp, ctx, X, nrm[:n], kp, R_SMALL)
        cloud.free()
        assert got.tobytes() == fresh.tobytes() and frames.tobytes() == frames_fresh.tobytes() and np.array_equal(counts, counts_fresh), name
        if name != "derived":
            assert got.tobytes() == small["got"].tobytes(), name
    assert ctx.arena_live() == before


@pytest.mark.parametrize("K,radius", [(6, None), (8, None), (66, None), (130, None), (66, 0.5), (130, 0.5), (258, 0.5)])
def test_mirrored_surface_takes_the_tie_walk(pcp, ctx, K, radius):
    """tests/test_shot_host.py derives the case: the keypoint is the centre of symmetry, so P = K / 2 exactly on both axes and the five
    medians decide.  With spread distances the bins of d2 leave a handful of candidates; on a sphere every d2 falls into one bin (or
    two), all K rows are candidates -- 66: one block of 64 and two left over; 130: the five ranks 63 .. 67 straddle a block; 258: more
    than SHOT_STAGE of them -- and the ranks come from rounding-level differences of d2 and from the rows of equal d2."""
    pts = _mirrored(K // 2, seed=40 + K, radius=radius)
    pts = pts[np.random.default_rng(K).permutation(K)]
    kp = np.r_[np.zeros((1, 3)), [[0.011, -0.007, 0.005]]]                          # the centre, and a keypoint beside it (no symmetry)
    nrm = _unit(np.random.default_rng(K + 1), K)
    ref = sc.lrf(pts, kp, 1.0)
    assert list(ref["counts"]) == [K, K] and ref["tie"][0].all() and ref["gap"].min() > 1e-3 and ref["sign_margin"].min() > 1e-9
    got, frames, counts = abi(pcp, ctx, pts, nrm, kp, 1.0)
    good = check_frames(frames, counts, ref)
    assert good.all()
    lrf, _ = abi_lrf(pcp, ctx, pts, kp, 1.0)
    assert lrf.tobytes() == frames.tobytes()
    check_values(got, frames, counts, pts, nrm, kp, 1.0)
    moved = _reordered(pcp, pts, ctx)
    relaid, f_r, _ = abi(pcp, ctx, moved, nrm, kp, 1.0)
    moved.free()
    assert relaid.tobytes() == got.tobytes() and f_r.tobytes() == frames.tobytes()


def test_a_row_at_the_keypoint_leaves_the_canonical_sign(pcp, ctx):
    """tests/test_shot_host.py derives the case: with the keypoint itself among the rows of the mirrored surface, s = 1 for both signs
    of both axes, and the frame is the one whose axes have their component of largest magnitude positive."""
    pts = np.r_[_mirrored(3, seed=21), np.zeros((1, 3))]
    kp = np.zeros((1, 3))
    ref = sc.lrf(pts, kp, 1.0)
    assert ref["counts"][0] == 7 and not ref["tie"].any()
    frames, counts = abi_lrf(pcp, ctx, pts, kp, 1.0)
    assert check_frames(frames, counts, ref).all()
    x, _, z = frames[0]
    assert x[np.argmax(np.abs(x))] > 0 and z[np.argmax(np.abs(z))] > 0


def test_rows_without_a_normal_are_skipped_on_both_sides(pcp, ctx, small):
    pts, kp = small["pts"], small["kp"]
    nrm = small["nrm"].copy()
    ball = pf.balls(pts, kp[:1], R_SMALL)[0]
    assert len(ball) > 10
    nrm[ball[[1, 4]]] = np.nan
    nrm[ball[7], 2] = np.inf
    got, frames, counts = abi(pcp, ctx, pts, nrm, kp, R_SMALL)
    assert frames.tobytes() == small["frames"].tobytes()                           # the frames do not read the normals
    assert np.abs(got[0] - small["got"][0]).max() > 1e-4                            # the case differs from the plain one
    ref = check_values(got, frames, counts, pts, nrm, kp, R_SMALL)
    assert ref["used"][0] <= ref["counts"][0] - 3


def test_unbounded_balls_succeed(pcp, ctx):
    """test_gpu_pcl_fpfh.py's cloud: 1 100 copies of one point (without a normal) and 6 rows beside it.  Every ball holds 1 106 rows;
    the keypoint whose ball holds the copies alone has a frame and no neighbour that is not skipped: a zero norm, 352 NaN."""
    rng = np.random.default_rng(41)
    c = np.array([1.0, 2.0, 3.0])
    pts = np.r_[np.tile([c], (1100, 1)), c + np.c_[rng.uniform(0.3, 0.5, 6), rng.uniform(-0.3, 0.3, (6, 2))]]
    nrm = _unit(rng, len(pts))
    nrm[:1100] = np.nan
    kp = np.r_[pts[1100:], pts[:1], [c - [0.75, 0.0, 0.0]]]
    before = ctx.arena_live()
    got, frames, counts = abi(pcp, ctx, pts, nrm, kp, 1.0)
    assert list(counts) == [1106] * 7 + [1100]
    assert np.isfinite(frames).all()
    ref = check_values(got, frames, counts, pts, nrm, kp, 1.0)
    assert list(ref["used"]) == [5] * 6 + [6, 0]
    assert np.isnan(got[7]).all() and np.isfinite(got[:7]).all()
    assert ctx.arena_live() == before


def test_far_and_nan_keypoints(pcp, ctx, small):
    pts, nrm = small["pts"], small["nrm"]
    kp = np.array([pts[0] + [1e3, 0.0, 0.0], [np.nan, 0.1, 0.1], [0.1, np.inf, 0.1], small["kp"][0]])
    got, frames, counts = abi(pcp, ctx, pts, nrm, kp, R_SMALL)
    assert list(counts[:3]) == [0, 0, 0] and np.isnan(got[:3]).all() and np.isnan(frames[:3]).all()
    assert got[3].tobytes() == small["got"][0].tobytes() and frames[3].tobytes() == small["frames"][0].tobytes()
    lrf, c2 = abi_lrf(pcp, ctx, pts, kp, R_SMALL)
    assert lrf.tobytes() == frames.tobytes() and np.array_equal(c2, counts)


def test_python_surface(pcp, ctx, small):
    pts, nrm, kp = small["pts"], small["nrm"], small["kp"]
    a, ia = pcp.shot352_with_normal(pts, nrm, kp, R_SMALL, ctx=ctx, return_info=True)
    assert a.dtype == np.float32 and a.shape == (len(kp), 352)
    assert a.tobytes() == small["got"].astype(np.float32).tobytes()                # the binary64 rounded once
    assert ia["frames"].tobytes() == small["frames"].tobytes() and ia["frames"].shape == (len(kp), 3, 3)
    assert np.array_equal(ia["counts"], small["counts"]) and ia["counts"].dtype == np.int32 and (ia["n"], ia["m"]) == (len(pts), len(kp))
    b = pcp.shot352_with_normal(pts, nrm, kp, R_SMALL, frames=ia["frames"], ctx=ctx)
    assert b.tobytes() == a.tobytes()
    lrf, counts = pcp.shot_lrf(pts, kp, R_SMALL, ctx=ctx, return_counts=True)
    assert lrf.tobytes() == small["frames"].tobytes() and np.array_equal(counts, small["counts"])
    assert pcp.shot_lrf(pts, kp, R_SMALL, ctx=ctx).shape == (len(kp), 3, 3)
    cloud = pcp.DeviceCloud.upload(pts, ctx)
    assert pcp.shot352_with_normal(cloud, nrm, kp, R_SMALL, ctx=ctx).tobytes() == a.tobytes()
    assert pcp.shot_lrf(cloud, kp, R_SMALL, ctx=ctx).tobytes() == lrf.tobytes()
    # featureSHOT352 = the k-nearest normals, then featureSHOT352WithNormal
    vp = (0.4, -0.3, 2.0)
    knn = pcp.estimate_normals_knn(cloud, 10, vp, ctx=ctx)
    e, ie = pcp.shot352(cloud, kp, 10, R_SMALL, viewpoint=vp, ctx=ctx, return_info=True)
    f, _ = pcp.shot352_with_normal(pts, knn, kp, R_SMALL, ctx=ctx, return_info=True)
    assert e.tobytes() == f.tobytes() and e.dtype == np.float32 and np.isfinite(e[:-2]).all() and np.isnan(e[-2:]).all()
    assert ie["frames"].tobytes() == small["frames"].tobytes()
    cloud.free()
    # keypointHarris3D's (K,4) rows as they are; no keypoints at all; the defaults are the wrapper's
    k4 = np.c_[kp[:5], np.ones(5)]
    assert pcp.shot352_with_normal(pts, nrm, k4, R_SMALL, ctx=ctx).tobytes() == a[:5].tobytes()
    none, info = pcp.shot352_with_normal(pts, nrm, [], R_SMALL, ctx=ctx, return_info=True)
    assert none.shape == (0, 352) and none.dtype == np.float32 and info["m"] == 0 and info["frames"].shape == (0, 3, 3)
    d = pcp.shot352(pts, kp[:4], ctx=ctx)
    g = pcp.shot352_with_normal(pts, pcp.estimate_normals_knn(pts, ctx=ctx), kp[:4], ctx=ctx)
    assert d.tobytes() == g.tobytes() and d.shape == (4, 352)


def test_errors_leave_nothing_behind(pcp, ctx, small):
    pts, nrm, kp = small["pts"], small["nrm"], small["kp"]
    L = pcp._lib
    before = ctx.arena_live()
    for bad_nrm, bad_kp, bad_frames in ((nrm[:-1], kp, None), (nrm, np.zeros((4, 2)), None), (nrm, kp, np.zeros((3, 9)))):
        with pytest.raises(ValueError):
            pcp.shot352_with_normal(pts, bad_nrm, bad_kp, R_SMALL, frames=bad_frames, ctx=ctx)
    for radius in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(L.PcrError) as e:
            pcp.shot352_with_normal(pts, nrm, kp, radius, ctx=ctx)
        assert e.value.status == L.PCR_E_INVALID
        with pytest.raises(L.PcrError) as e:
            pcp.shot_lrf(pts, kp, radius, ctx=ctx)
        assert e.value.status == L.PCR_E_INVALID
    cloud = pcp.DeviceCloud.upload(pts, ctx)
    held = ctx.arena_live()
    out = np.full((2, 352), -7.0)
    fr = np.full((2, 9), -7.0)
    k2 = np.ascontiguousarray(kp[:2])
    nr = np.ascontiguousarray(nrm)
    f, g = L.lib().pcr_shot352, L.lib().pcr_shot_lrf
    assert f(ctx.handle, cloud.handle, L.dptr(nr), L.dptr(k2), -1, R_SMALL, None, L.dptr(out), None, None) == L.PCR_E_INVALID
    assert f(ctx.handle, cloud.handle, L.dptr(nr), L.dptr(k2), 2 ** 31, R_SMALL, None, L.dptr(out), None, None) == L.PCR_E_INVALID
    assert f(ctx.handle, cloud.handle, None, L.dptr(k2), 2, R_SMALL, None, L.dptr(out), None, None) == L.PCR_E_INVALID
    assert f(ctx.handle, cloud.handle, L.dptr(nr), None, 2, R_SMALL, None, L.dptr(out), None, None) == L.PCR_E_INVALID
    assert f(ctx.handle, cloud.handle, L.dptr(nr), L.dptr(k2), 2, R_SMALL, None, None, None, None) == L.PCR_E_INVALID
    assert f(ctx.handle, None, L.dptr(nr), L.dptr(k2), 2, R_SMALL, None, L.dptr(out), None, None) == L.PCR_E_INVALID
    assert g(ctx.handle, cloud.handle, L.dptr(k2), -1, R_SMALL, L.dptr(fr), None) == L.PCR_E_INVALID
    assert g(ctx.handle, cloud.handle, None, 2, R_SMALL, L.dptr(fr), None) == L.PCR_E_INVALID
    assert g(ctx.handle, cloud.handle, L.dptr(k2), 2, R_SMALL, None, None) == L.PCR_E_INVALID
    assert (out == -7.0).all() and (fr == -7.0).all() and ctx.arena_live() == held
    assert f(ctx.handle, cloud.handle, L.dptr(nr), L.dptr(k2), 0, R_SMALL, None, L.dptr(out), L.dptr(fr), None) == L.PCR_OK       # m = 0: nothing written
    assert g(ctx.handle, cloud.handle, L.dptr(k2), 0, R_SMALL, L.dptr(fr), None) == L.PCR_OK
    assert (out == -7.0).all() and (fr == -7.0).all()
    assert f(ctx.handle, cloud.handle, L.dptr(nr), L.dptr(k2), 2, R_SMALL, None, L.dptr(out), None, None) == L.PCR_OK              # the optional outputs may be NULL
    assert out.tobytes() == small["got"][:2].tobytes()
    assert g(ctx.handle, cloud.handle, L.dptr(k2), 2, R_SMALL, L.dptr(fr), None) == L.PCR_OK
    assert fr.tobytes() == small["frames"][:2].tobytes()
    cloud.free()
    # a cloud whose extent exceeds 2^18 radii
    wide = np.r_[pts, [[3.0e5, 0.0, 0.0]]]
    with pytest.raises(L.PcrError) as e:
        pcp.shot352_with_normal(wide, np.r_[nrm, [[0.0, 0.0, 1.0]]], kp, 1.0, ctx=ctx)
    assert e.value.status == L.PCR_E_UNSUPPORTED and b"2^18" in L.lib().pcr_last_error(ctx.handle)
    with pytest.raises(L.PcrError) as e:
        pcp.shot_lrf(wide, kp, 1.0, ctx=ctx)
    assert e.value.status == L.PCR_E_UNSUPPORTED
    got, _, _ = abi(pcp, ctx, pts, nrm, kp, R_SMALL)
    assert got.tobytes() == small["got"].tobytes()
    assert ctx.arena_live() == before
