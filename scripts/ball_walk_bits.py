"""One SHA-256 per output of every call that walks a radius ball through csrc/pcr_ball_visit.h (and of the calls whose wave sums go
through csrc/pcr_wave.h's wave_sum_all), on fixed seeded inputs, for the library in PCR_LIB_PATH (default: the built one).  Two
libraries compute the same bits if and only if their outputs are identical line for line:

    python scripts/ball_walk_bits.py > a.txt;  PCR_LIB_PATH=/path/to/other/libpcr.so python scripts/ball_walk_bits.py > b.txt;  diff a.txt b.txt

Calls: estimate_normals_radius (with counts), keypointHarris3D (every row with details; suppressed and refined with details), keypointIss,
iss_keypoints (device suppression: iss_count 20; host suppression: iss_count 2000), estimate_normals (k = 3, 10, 16),
estimate_normals_knn, estimate_normals_hybrid, compute_fpfh_feature, compute_fpfh_at_rows, fpfh33, fpfh33_with_normal -- each on a
fresh upload and on a cloud prepared for an index -- and ransac_init (host clouds, detectors voxel and harris) for pcr_ransac's sum.
Inputs: n = 1, 2, 65, 1 500 and 20 000 rows of synthetic.kitti_like_scan; the 5 x 5 x 5 unit lattice at radius 1 (rows exactly on the
radius); tests/ball_walk_checks.py's built cloud, whose balls have 1, 2, 63, 64, 65, 127, 128, 129, 192, 193, 256 and 257 rows (asserted on
the restatement before anything is hashed).  The FPFH33 keypoints: rows of the cloud, two positions outside its box by 0.5 r and by
2 r, and one that is not finite.  An error is an output too: its type and text are hashed like a result.
"""
import hashlib
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pcp = importlib.import_module("point-cloud-process_amd")
from tests import ball_walk_checks as bw  # noqa: E402
from tests import harris_checks as hc  # noqa: E402

SCAN_SIZES = (1, 2, 65, 1500, 20000)
RADIUS, NON_MAX, THRESHOLD, GAMMA, MIN_NB, MAX_NN = 1.0, 0.7, 0.001, 0.975, 5, 100


def emit(name, *values):
    h = hashlib.sha256()
    for v in values:
        a = np.ascontiguousarray(v)
        if a.dtype == object:   # (nothing returns one today; its bytes would be addresses)
            a = np.frombuffer(repr(v).encode(), dtype=np.uint8)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    print(f"{name} {h.hexdigest()}", flush=True)


def attempt(name, fn):
    try:
        emit(name, *fn())
    except Exception as e:   # noqa: BLE001 -- the error is the output
        emit(name + " raised", np.frombuffer(f"{type(e).__name__}: {e}".encode(), dtype=np.uint8))


def details(d):
    return [d[k] for k in sorted(d)]


def keypoint_positions(points, r):
    lo, hi = points.min(axis=0), points.max(axis=0)
    rows = np.random.default_rng(41 * len(points)).choice(len(points), min(len(points), 200), replace=False)
    extra = np.array([hi + 0.5 * r, lo - 2.0 * r, [np.nan, 0.0, 0.0]])
    return rows, np.concatenate([points[rows], extra])


def cloud_calls(tag, points, r, dc, ctx):
    n = len(points)
    rows, kp = keypoint_positions(points, r)
    attempt(tag + " estimate_normals_radius", lambda: pcp.estimate_normals_radius(dc, r, ctx=ctx, return_counts=True))

    def harris(**kw):
        out = pcp.keypointHarris3D(dc, radius=r, nms_threshold=THRESHOLD, return_indices=True, return_details=True, ctx=ctx, **kw)
        return [out[0], out[1]] + details(out[2])
    attempt(tag + " keypointHarris3D", harris)
    attempt(tag + " keypointHarris3D nms refine", lambda: harris(is_nms=True, is_refine=True))

    def iss_pcl():
        out = pcp.keypointIss(dc, r, NON_MAX * r, GAMMA, GAMMA, MIN_NB, return_indices=True, return_details=True, ctx=ctx)
        return [out[0], out[1]] + details(out[2])
    attempt(tag + " keypointIss", iss_pcl)
    for what, count in (("device nms", 20), ("host nms", 2000)):
        def iss():
            idx, lam, counts = pcp.iss_keypoints(dc, radius=r, non_max_radius=r, iss_count=count, ctx=ctx, return_details=True)
            return np.asarray(idx, dtype=np.int64), lam, counts
        attempt(f"{tag} iss_keypoints {what}", iss)
    for k in (3, 10, 16):
        attempt(f"{tag} estimate_normals k={k}", lambda: pcp.estimate_normals(dc, k, ctx=ctx, return_details=True))
    attempt(tag + " estimate_normals_knn", lambda: pcp.estimate_normals_knn(dc, 10, return_curvature=True, ctx=ctx))
    hybrid = []
    attempt(tag + " estimate_normals_hybrid", lambda: hybrid.append(pcp.estimate_normals_hybrid(dc, r, 30, ctx=ctx)) or hybrid)
    if hybrid:
        attempt(tag + " compute_fpfh_feature", lambda: [pcp.compute_fpfh_feature(dc, hybrid[0], r, MAX_NN, ctx=ctx).data])

        def at_rows():
            f, info = pcp.compute_fpfh_at_rows(dc, rows, hybrid[0], r, MAX_NN, ctx=ctx, return_info=True)
            return [f.data] + details(info)
        attempt(tag + " compute_fpfh_at_rows", at_rows)

    def fpfh33():
        f, info = pcp.fpfh33(dc, kp, 10, r, ctx=ctx, return_info=True)
        return [f] + details(info)
    attempt(tag + " fpfh33", fpfh33)

    def fpfh33_wn():
        nrm = np.random.default_rng(43 * n).normal(size=(n, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        nrm[:: 17] = np.nan   # rows without a normal
        f, info = pcp.fpfh33_with_normal(dc, nrm, kp, r, ctx=ctx, return_info=True)
        return [f] + details(info)
    attempt(tag + " fpfh33_with_normal", fpfh33_wn)


def main():
    ctx = pcp.default_context()
    built = bw.built_cloud()
    sizes = np.array([len(b) for b in hc.neighbours(built, bw.BUILT_RADIUS)])
    assert set(bw.BALL_SIZES) <= set(sizes.tolist()), sorted(set(sizes.tolist()))
    inputs = [(f"scan n={n}", pcp.synthetic.kitti_like_scan(n, seed=11)[:, :3].astype(np.float64), RADIUS) for n in SCAN_SIZES]
    inputs += [("lattice", bw.lattice(), 1.0), ("built", built, bw.BUILT_RADIUS)]
    index = pcp.TargetIndex(pcp.synthetic.kitti_like_scan(20000, seed=7).astype(np.float64), kind="grid", ctx=ctx)   # what `prepared` clouds are laid out for
    for name, points, r in inputs:
        points = np.ascontiguousarray(points)
        for layout in ("uploaded", "prepared"):
            dc = pcp.DeviceCloud.upload(points, ctx)
            if layout == "prepared":
                dc.prepare(index)
            cloud_calls(f"{name} {layout}", points, r, dc, ctx)
            dc.free()
    index.free()
    src, tgt, _ = pcp.synthetic.perturbed_pair(20000, seed=3)
    for detector in ("voxel", "harris"):
        def init():
            R, t, info = pcp.ransac_init(src.astype(np.float64), tgt.astype(np.float64), 2.0, seed=0, ctx=ctx, detector=detector, return_info=True)
            return R, t, np.float64(info["fitness"]), np.float64(info["inlier_rmse"])
        attempt(f"ransac_init {detector}", init)


if __name__ == "__main__":
    main()
